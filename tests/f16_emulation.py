"""The float64 EMULATION of backend 'hip_f16'  that tests/test_gpu_conv_f16.py and tests/test_gpu_pnp_f16.py hold the kernels
to: PyTorch in float64, rounding to IEEE half exactly where the backend rounds.  Not a test module."""
import copy


def emulation(D, torch, net64):
    """a float64 copy of the network that rounds where backend 'hip_f16' rounds: weights of every layer but the first to half; the result
    of every layer but the last to half (rounding commutes with the ReLU behind a convolution; a residual block rounds after its skip
    sum); the operand of a layer that consumes a skip sum (transposed convolutions, the U-Net's last layer) to half"""
    net = copy.deepcopy(net64)
    rnd = lambda t: t.half().double()
    convs = [m for m in net.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d))]
    first, last = convs[0], convs[-1]
    if isinstance(net, D.UNetRes):
        first, last = net.m_head, net.m_tail
    with torch.no_grad():
        for m in convs:
            if m is not first:
                m.weight.copy_(rnd(m.weight))
    second_of_block = {id(b.res[2]) for b in net.modules() if isinstance(b, D._ResBlock)}
    for m in convs:
        if m is not last and id(m) not in second_of_block:
            m.register_forward_hook(lambda mod, inp, out: rnd(out))
        if isinstance(m, torch.nn.ConvTranspose2d) or (m is last and isinstance(net, D.UNetRes)):
            m.register_forward_pre_hook(lambda mod, inp: (rnd(inp[0]),))
    for b in net.modules():
        if isinstance(b, D._ResBlock):
            b.register_forward_hook(lambda mod, inp, out: rnd(out))
    return net
