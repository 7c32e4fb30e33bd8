// paper_rules.hpp — paper mode's per-pixel rules, written once for every
// caller: the frame kernels' finish pass (rt_kernels.hpp paper_pixel), the
// stencil over a caller's G-buffer (rt_paper_f64.hip k_paper_resolve) and the
// host form of rt_paper_resolve (rt_host.cpp).  Functions of plain values
// only: no scene, no record layout, no memory access.  R is the arithmetic
// type (double everywhere but the FP32 diagnostic frames).  Every translation
// unit that includes this is compiled without FP contraction.
//
//   get_luminance     tracer.cpp:123-125
//   get_edge_strength tracer.cpp:133-178
//   apply_crosshatch  tracer.cpp:188-205 (in two halves: hatch_band, crosshatch)
//   the pixel         tracer.cpp:266-279
#pragma once

#if defined(__HIPCC__)
#define RT_RULES_FN __host__ __device__ __forceinline__
#else
#define RT_RULES_FN inline
#endif

namespace rtamd {
namespace paper {

// std::max / std::min: (a < b) ? b : a and (b < a) ? b : a, so a NaN in the
// second place is dropped and one in the first place stays.
template <class R>
RT_RULES_FN R rmax(R a, R b) { return (a < b) ? b : a; }
template <class R>
RT_RULES_FN R rmin(R a, R b) { return (b < a) ? b : a; }

// get_luminance: left to right, every product and sum rounded once.
template <class R>
RT_RULES_FN R luminance(R r, R g, R b) {
    return static_cast<R>(0.299) * r + static_cast<R>(0.587) * g + static_cast<R>(0.114) * b;
}

// apply_crosshatch's FP part, the luminance tests, reduced to a band (0:
// lum < 0.15, black; 1..6: the darkness branch taken; 7: no branch, white; a
// NaN luminance takes none, as in the reference).
template <class R>
RT_RULES_FN int hatch_band(R lum) {
    if (lum < static_cast<R>(0.15)) return 0;
    const R darkness = static_cast<R>(1.0) - lum;
    if (darkness > static_cast<R>(0.8)) return 1;
    if (darkness > static_cast<R>(0.65)) return 2;
    if (darkness > static_cast<R>(0.5)) return 3;
    if (darkness > static_cast<R>(0.35)) return 4;
    if (darkness > static_cast<R>(0.2)) return 5;
    if (darkness > static_cast<R>(0.12)) return 6;
    return 7;
}
// ... and its integer part, the band's (x, y) pattern: 0 = ink, 1 = paper.
// C++ '%' truncates toward zero ((x - y) % 4 may be negative).
template <class R>
RT_RULES_FN R crosshatch(int band, int x, int y) {
    if (band == 0) return static_cast<R>(0.0);
    const bool diag1 = ((x + y) % 4) < 1;
    const bool diag2 = ((x - y) % 4) < 1;
    const bool horizontal = (y % 4) < 1;
    bool draw = false;
    if (band == 1) draw = (diag1 && diag2) || horizontal;
    else if (band == 2) draw = (diag1 && diag2) || (horizontal && ((x + y) % 3 == 0));
    else if (band == 3) draw = (diag1 && diag2) || (horizontal && ((x + y) % 4 == 0));
    else if (band == 4) draw = diag1 || (horizontal && ((x + y) % 3 == 0));
    else if (band == 5) draw = diag1;
    else if (band == 6) draw = diag1 && ((x + y) % 8) < 2;
    return draw ? static_cast<R>(0.0) : static_cast<R>(1.0);
}

// get_edge_strength from the centre's record and its four neighbours', in the
// reference's order (-1,0) (1,0) (0,-1) (0,1).  ch / nh: the hit flags; nv: the
// neighbour lies inside the frame (one outside is skipped and not counted).
// Material identity is the index (two -1 are equal, as two null pointers are).
// Returns the edge strength; eidx is its index in {0, 0.3, 0.5, 0.6, 0.9}
// before the halving and valid the number of neighbours counted (the
// distributed frames' output alphabet, rtamd::paper_code).
template <class R>
RT_RULES_FN R edge_strength(bool ch, R ct, R cnx, R cny, R cnz, int cm, const bool (&nv)[4], const bool (&nh)[4],
                            const R (&nt)[4], const R (&nnx)[4], const R (&nny)[4], const R (&nnz)[4],
                            const int (&nm)[4], int& eidx, int& valid) {
    R maxEdge = static_cast<R>(0.0);
    eidx = 0;
    valid = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) {
        if (!nv[i]) continue;
        ++valid;
        if (ch != nh[i]) {
            maxEdge = rmax(maxEdge, static_cast<R>(0.9));
            eidx = eidx < 4 ? 4 : eidx;
            continue;
        }
        if (ch && nh[i]) {
            const R minD = rmin(ct, nt[i]), maxD = rmax(ct, nt[i]);
            if (minD > static_cast<R>(1e-4) && maxD / minD > static_cast<R>(3.0)) {
                maxEdge = rmax(maxEdge, static_cast<R>(0.6));
                eidx = eidx < 3 ? 3 : eidx;
            }
            const R nd = cnx * nnx[i] + cny * nny[i] + cnz * nnz[i];
            if (nd < static_cast<R>(0.2)) {
                maxEdge = rmax(maxEdge, static_cast<R>(0.5));
                eidx = eidx < 2 ? 2 : eidx;
            }
            if (cm != nm[i] && nd < static_cast<R>(0.7)) {
                maxEdge = rmax(maxEdge, static_cast<R>(0.3));
                eidx = eidx < 1 ? 1 : eidx;
            }
        }
    }
    if (valid < 4) maxEdge *= static_cast<R>(0.5);
    return maxEdge;
}

// The pixel of tracer.cpp:267-278 from its edge strength and hatch band; the
// three channels are equal.
template <class R>
RT_RULES_FN R pixel_value(R edge, int band, int x, int y) {
    if (edge > static_cast<R>(0.8)) return static_cast<R>(0.0);
    if (edge > static_cast<R>(0.5)) return static_cast<R>(0.2);
    R o = crosshatch<R>(band, x, y);
    if (edge > static_cast<R>(0.3)) {
        const R darken = (edge - static_cast<R>(0.3)) * static_cast<R>(0.4);
        o *= (static_cast<R>(1.0) - darken);
    }
    return o;
}

}  // namespace paper
}  // namespace rtamd
