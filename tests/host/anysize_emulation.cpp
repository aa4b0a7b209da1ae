// CPU emulation of the any-size FFT (csrc/kernels_anysize.hip) from the header the kernels include (csrc/anysize_plan.h):
// the plan, the fp64 tables and one line transform, forward and inverse, in the order line_fft runs them.
//   anysize_emulation <n> <in.bin> <out.bin>
//   in : n complex128 (x)
//   out: int32 n, bluestein, m, nstages, radix[12]; complex128 tw[m], chirp[n], kern[m] (zeros unless Bluestein);
//        complex128 fwd[n], inv[n] (unnormalised)
#include "../../pnp_admm_cnc_mri_amd/csrc/anysize_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace pnp::anysize;

struct cd { double x, y; };

// line_fft of the kernels, one line, serial
template <bool INV>
static std::vector<cd> line(const Plan& p, const std::vector<cd>& tw, const std::vector<cd>& ch, const std::vector<cd>& kern,
                            const std::vector<cd>& x) {
    std::vector<cd> a(p.m + 1), b(p.m + 1);
    for (int j = 0; j < p.n; ++j) a[j] = x[j];
    if (!p.bluestein) {
        cd* r = stockham_host<INV>(a.data(), b.data(), tw.data(), p.radix, p.nstages, p.m);
        return std::vector<cd>(r, r + p.n);
    }
    for (int j = 0; j < p.m; ++j) {
        cd v = mkc<cd>(0.0, 0.0);
        if (j < p.n) { v = a[j]; if (INV) v = cconj(v); v = cmul(v, ch[j]); }
        a[j] = v;
    }
    cd* r = stockham_host<false>(a.data(), b.data(), tw.data(), p.radix, p.nstages, p.m);
    cd* o = (r == a.data()) ? b.data() : a.data();
    for (int j = 0; j < p.m; ++j) r[j] = cmul(r[j], kern[j]);
    r = stockham_host<true>(r, o, tw.data(), p.radix, p.nstages, p.m);
    std::vector<cd> out(p.n);
    for (int j = 0; j < p.n; ++j) { cd v = cmul(r[j], ch[j]); out[j] = INV ? cconj(v) : v; }
    return out;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int n = atoi(argv[1]);
    const Plan p = make_plan(n);
    if (p.nstages < 1) return 3;
    std::vector<cd> x(n);
    FILE* f = fopen(argv[2], "rb");
    if (!f || fread(x.data(), sizeof(cd), n, f) != (size_t)n) return 4;
    fclose(f);
    std::vector<double> tre, tim, cre, cim;
    twiddles(p.m, tre, tim);
    std::vector<cd> tw(p.m), ch(n, mkc<cd>(0.0, 0.0)), kern(p.m, mkc<cd>(0.0, 0.0));
    for (int i = 0; i < p.m; ++i) tw[i] = mkc<cd>(tre[i], tim[i]);
    if (p.bluestein) {
        chirp(n, cre, cim);
        for (int j = 0; j < n; ++j) ch[j] = mkc<cd>(cre[j], cim[j]);
        bluestein_kernel<cd>(p, cre, cim, kern);
    }
    const std::vector<cd> fwd = line<false>(p, tw, ch, kern, x), inv = line<true>(p, tw, ch, kern, x);
    f = fopen(argv[3], "wb");
    if (!f) return 5;
    const int hdr[4] = {p.n, p.bluestein, p.m, p.nstages};
    fwrite(hdr, sizeof(int), 4, f);
    fwrite(p.radix, sizeof(int), MAX_STAGES, f);
    const std::vector<cd>* parts[] = {&tw, &ch, &kern, &fwd, &inv};
    for (const std::vector<cd>* v : parts) fwrite(v->data(), sizeof(cd), v->size(), f);
    fclose(f);
    return 0;
}
