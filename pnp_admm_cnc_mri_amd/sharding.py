"""Slice sharding across the GPUs of one node.

Every slice has its own (y, mask, z, w): there is no cross-slice term anywhere in the
reference (its outer `for` over images, S4:83, carries no state), so N processes -- one per
GPU, `torch.distributed` over RCCL -- each run the whole ADMM loop on a contiguous block of
slices with ZERO communication, and one gather of the float32 reconstructions ends the job.

On the MI355X xGMI mesh every peer has its own link to the root, so the gather is issued as
one direct `dist.gather` (peers -> root in parallel, 7 links), not a ring.
Works with backend "nccl" (= RCCL, device tensors) and "gloo" (CPU tensors; used by the
world_size-2 tests).
"""
import numpy as np


def shard_range(B, world, rank):
    """Contiguous block [lo, hi) of rank `rank`: sizes differ by at most one, earlier ranks larger."""
    if world < 1 or not (0 <= rank < world):
        raise ValueError('bad world/rank %d/%d' % (world, rank))
    base, rem = divmod(B, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_sizes(B, world):
    return [shard_range(B, world, r)[1] - shard_range(B, world, r)[0] for r in range(world)]


def gather_slices(x_local, B_total, dst=0, group=None):
    """x_local: torch tensor [b_r, H, W] of this rank (device tensor for nccl, CPU for gloo).
    Returns the [B_total, H, W] tensor on `dst` (None elsewhere).

    The root receives into ONE [world * bmax, H, W] tensor whose per-rank views are the gather
    list, so even shards (the benchmark's and every power-of-two job's case) need no second copy
    of the result: the tensor returned IS the receive buffer.  Uneven shards are padded to the
    largest shard for the collective and compacted on the root.  A complex tensor (image='complex') travels as its real view
    [b_r, H, W, 2] -- dist.gather takes no complex dtype -- and comes back complex on the root."""
    import torch
    import torch.distributed as dist
    if x_local.is_complex():
        out = gather_slices(torch.view_as_real(x_local.contiguous()), B_total, dst=dst, group=group)
        return None if out is None else torch.view_as_complex(out.contiguous())
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)                       # position inside `group`: which shard this rank holds
    # `dst` is a GLOBAL rank (what dist.gather takes), so compare it with the global rank
    is_dst = dist.get_rank() == dst
    sizes = shard_sizes(B_total, world)
    if x_local.shape[0] != sizes[rank]:
        raise ValueError('rank %d holds %d slices, expected %d' % (rank, x_local.shape[0], sizes[rank]))
    bmax = max(sizes)
    send = x_local.contiguous()
    if send.shape[0] != bmax:
        pad = torch.zeros((bmax,) + tuple(send.shape[1:]), dtype=send.dtype, device=send.device)
        pad[:send.shape[0]] = send
        send = pad
    recv, bufs = None, None
    if is_dst:
        recv = torch.empty((world * bmax,) + tuple(send.shape[1:]), dtype=send.dtype, device=send.device)
        bufs = [recv[r * bmax:(r + 1) * bmax] for r in range(world)]     # contiguous views: the collective fills `recv` in place
    dist.gather(send, bufs, dst=dst, group=group)
    if not is_dst:
        return None
    if all(n == bmax for n in sizes):
        return recv
    return torch.cat([bufs[r][:sizes[r]] for r in range(world)], dim=0)


def run_sharded(solve_shard, B_total, group=None, dst=0):
    """solve_shard(lo, hi) -> torch tensor [hi-lo, H, W]; runs it on this rank's block and gathers.
    With no process group initialised it is a plain single-process call."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return solve_shard(0, B_total)
    lo, hi = shard_range(B_total, dist.get_world_size(group), dist.get_rank(group))
    return gather_slices(solve_shard(lo, hi), B_total, dst=dst, group=group)


def solve_sharded(solver, mask, noises, images=None, y=None, mask_id=None, dst=0, group=None, gather_device=None, coil_id=None,
                  **solver_kwargs):
    """Run one of the entry points (ADMM_L1, ADMM_CNC, PNP_ADMM_*_D: anything with the
    `(…, mask, noises, images=, y=, mask_id=, **opts) -> out | (out, …)` shape, pre-bound with
    `functools.partial` when it takes leading model names) on this rank's contiguous block of slices
    and gather the reconstructions on `dst`.

    coil_id [B] (with coils= among the solver's keywords: a bank of coil maps, which every rank gets whole) is sliced with the shard as
    mask_id is, and so is per-slice noise -- [B,H,W] without coils, [B,C,H,W] with them ([C,H,W] is shared by the slices).
    Every rank passes the SAME full `images` / `y` / `mask_id` / `coil_id`; returns an array [B_total, H, W] on `dst`
    (float32; float64 when the solver is run with precision='f64'; complex64 / complex128 with image='complex'), None elsewhere.  With no process
    group it is a plain call.
    gather_device: torch device for the collective (default under nccl: the device the solver's result lies on -- see
    collective_device; cpu under gloo).  Solver contract: called as solver(mask, noises, images=/y=/mask_id= slices, **opts,
    return_device=True when its signature takes that keyword) and returns a [b,H,W] tensor or the reference's list (+ extras in a tuple).
    """
    import torch
    import torch.distributed as dist
    src = images if images is not None else y
    if src is None:
        raise ValueError('solve_sharded needs images= or y= (file-based inputs cannot be sharded by index)')
    B_total = len(src)
    grouped = dist.is_available() and dist.is_initialized()
    frames = solver_kwargs.get('frames')
    if frames is not None:
        # temporal sparsity: a series is `frames` consecutive slices and the blocks below would cut one in two.  Every rank judges every
        # shard -- its own or not, before any work -- so all of them raise the same error and none is left waiting in the gather
        from .engine import check_temporal
        check_temporal(frames)
        sizes = shard_sizes(B_total, dist.get_world_size(group) if grouped else 1)
        if any(n % int(frames) for n in sizes):
            raise ValueError('solve_sharded: frames=%d does not divide the shards %s of %d slices over %d ranks: a series would be cut in two '
                             '(series-aligned splitting is not built; choose a batch of ranks x k x frames slices)'
                             % (int(frames), sizes, B_total, len(sizes)))
    if not grouped:
        lo, hi = 0, B_total
    else:
        lo, hi = shard_range(B_total, dist.get_world_size(group), dist.get_rank(group))
    kw = dict(solver_kwargs)
    real = np.float64 if kw.get('precision') == 'f64' else np.float32
    if images is not None:
        kw['images'] = np.asarray(images)[lo:hi]
    if y is not None:
        kw['y'] = np.asarray(y)[lo:hi]
    if mask_id is not None:
        kw['mask_id'] = np.asarray(mask_id)[lo:hi]
    if coil_id is not None:
        kw['coil_id'] = np.asarray(coil_id)[lo:hi]
    per_slice_ndim = 3 if kw.get('coils') is None else 4
    if noises is not None and np.ndim(noises) == per_slice_ndim:       # per-slice k-space noise [B,H,W] ([B,C,H,W] with coils): shard it with the slices
        noises = np.asarray(noises)[lo:hi]
    # The reconstructions stay on the device between the solver and the collective: `return_device=True` makes the entry point
    # hand back ONE [b,H,W] device tensor (no 22-slot list of host arrays), RCCL gathers it as it is, and the only device-to-host
    # copy of the job is the root's, of the gathered result (config 4: 128 MiB per rank stay off PCIe in both directions).
    tdt = torch.float64 if real is np.float64 else torch.float32
    if _bound(solver, 'image') == 'complex' and kw.get('image') != 'complex':        # known before anything runs
        raise TypeError("solve_sharded: image='complex' is bound into the solver with functools.partial but is not among solve_sharded's "
                        'keywords (every rank, also one with an empty shard, must know the dtype of the gather): pass it there')
    if kw.get('image') == 'complex':                      # all five solvers with image='complex': the gathered array is complex
        real = np.complex128 if real is np.float64 else np.complex64
        tdt = torch.complex128 if real is np.complex128 else torch.complex64
    if hi > lo:
        # solver contract: `return_device=True` -> ONE [b,H,W] tensor (every entry point of this package); a solver whose signature has
        # neither that keyword nor **opts is called without it and may return the reference's list of host arrays
        res = solver(mask, noises, **(dict(kw, return_device=True) if _accepts(solver, 'return_device') else kw))
        out = res[0] if isinstance(res, tuple) else res
        if torch.is_tensor(out):
            x_local = out
        else:                                             # a solver that keeps the reference's list of host arrays whatever it is asked
            x_local = torch.from_numpy(np.stack([np.asarray(out[n], dtype=real) for n in range(hi - lo)]))
        if tuple(x_local.shape[:1]) != (hi - lo,):
            raise TypeError('solve_sharded: the solver returned %s for a shard of %d slices' % (tuple(x_local.shape), hi - lo))
        if x_local.is_complex() and not tdt.is_complex:   # e.g. image='complex' bound with functools.partial: a cast would drop the phase
            raise TypeError("solve_sharded: the solver returned a complex result but image='complex' is not among solve_sharded's "
                            'keywords (every rank, also one with an empty shard, must know the dtype of the gather): pass it there')
        if x_local.dtype != tdt:                          # one dtype on every rank (empty shards send zeros of `tdt`): mixed dtypes hang a gather
            x_local = x_local.to(tdt)
    else:
        m = np.asarray(mask)
        x_local = torch.zeros((0,) + tuple(m.shape[-2:]), dtype=tdt)
    if not grouped:
        return x_local.cpu().numpy()
    if gather_device is None:                             # (a one-rank group still runs the collective: RCCL's first contact is a test)
        gather_device = collective_device(x_local, dist.get_backend(group), kw.get('device'))
    x_all = gather_slices(x_local.to(gather_device), B_total, dst=dst, group=group)     # .to(): a no-op for a tensor already there
    return None if x_all is None else x_all.cpu().numpy()


def collective_device(x_local, backend, device=None):
    """Where the final gather runs.  gloo: the CPU.  nccl (= RCCL): the card the shard's result already lies on -- the solver may have
    been bound to its device with functools.partial (then `device` never reaches solve_sharded's keywords), and RCCL must be handed
    a tensor on THIS rank's GPU, never a copy onto the root's.  A CPU tensor (an empty shard, a list-returning solver) goes to the
    explicit device=, else to the process's LOCAL_RANK (solvers.resolve_device)."""
    import torch
    if backend != 'nccl':
        return torch.device('cpu')
    if x_local.is_cuda:
        return x_local.device
    from .solvers import resolve_device
    return torch.device('cuda', resolve_device(device))


def _bound(fn, name):
    """the value a chain of functools.partial binds to the keyword `name` (the outermost wins), None when none does"""
    import functools
    while isinstance(fn, functools.partial):
        if name in fn.keywords:
            return fn.keywords[name]
        fn = fn.func
    return None


def _accepts(fn, name):
    """does `fn` (possibly a functools.partial) take the keyword `name`, by name or through **kwargs?"""
    import inspect
    try:
        ps = inspect.signature(fn).parameters.values()
    except (TypeError, ValueError):
        return True
    return any(p.name == name or p.kind is inspect.Parameter.VAR_KEYWORD for p in ps)
