// mfx_half.h — the FP16 node image of the per-lane trace kernels (MfxNodeH, mfx_layout.h), made on the
// host from the FP32 nodes: mfx_api.cpp uploads it, scene_digest.cpp pins its rounding and its bytes on
// a machine without a GPU. Host only.
#ifndef MFX_HALF_H
#define MFX_HALF_H

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "mfx_layout.h"

namespace mfx_half {

// IEEE binary16 bits of the half nearest x in the direction `up` (true: the least half >= x, false:
// the greatest half <= x); beyond the half range: +-inf on the outward side, +-65504 on the inward
inline uint16_t half_dir(float x, bool up) {
    if (std::isinf(x)) return x > 0 ? 0x7c00 : 0xfc00;
    if (x < 0) return (uint16_t)(0x8000 | half_dir(-x, !up));
    if (x == 0) return up ? 0 : 0;
    if (x > 65504.f) return up ? 0x7c00 : 0x7bff;
    int e = 0;
    (void)std::frexp((double)x, &e);  // x = m * 2^e, m in [0.5, 1)
    const int ex = std::max(e - 1, -14);  // the half's exponent (subnormals: -14)
    const double ulp = std::ldexp(1.0, ex - 10);
    const double m = (double)x / ulp;  // exact (a power-of-two scaling)
    const double k = up ? std::ceil(m) : std::floor(m);
    const double v = k * ulp;  // representable (k <= 2048)
    if (v > 65504.0) return 0x7c00;
    if (v < std::ldexp(1.0, -14)) return (uint16_t)(v / std::ldexp(1.0, -24));  // subnormal
    int ve = 0;
    const double vm = std::frexp(v, &ve);  // v = vm * 2^ve
    const int E = ve - 1;
    const int mant = (int)((vm * 2.0 - 1.0) * 1024.0);
    return (uint16_t)(((E + 15) << 10) | mant);
}
// the per-lane kernels' FP16 node: each child's box rounded outward, empty children all +inf
inline MfxNodeH node_to_half(const MfxNode& n) {
    MfxNodeH h;
    for (int k = 0; k < 4; ++k) {
        const bool empty = n.child[k] == MFX_CHILD_EMPTY;
        h.lox[k] = empty ? 0x7c00 : half_dir(n.lox[k], false);
        h.hix[k] = empty ? 0x7c00 : half_dir(n.hix[k], true);
        h.loy[k] = empty ? 0x7c00 : half_dir(n.loy[k], false);
        h.hiy[k] = empty ? 0x7c00 : half_dir(n.hiy[k], true);
        h.loz[k] = empty ? 0x7c00 : half_dir(n.loz[k], false);
        h.hiz[k] = empty ? 0x7c00 : half_dir(n.hiz[k], true);
        h.child[k] = n.child[k];
    }
    return h;
}

}  // namespace mfx_half

#endif
