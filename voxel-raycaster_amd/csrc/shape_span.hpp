// shape_span.hpp -- the closed form behind the shape fills (vrc_fill_shapes, include/vrc.h; region_write.hip): which voxels of a
// row, and which bricks of a brick row, a ball or an axis-aligned cylinder holds.  Membership is defined in integers, so nothing
// here rounds: an axis with |d| > r is outside and is tested first, after which every square is at most 2^60 and every sum fits
// signed 64 bits.  A header of its own because it compiles for the host as it stands: tests/shape_span_check.cpp holds it against
// per-voxel membership on the CPU.
//
//   kind 0      ball:      (x - cx)^2 + (y - cy)^2 + (z - cz)^2 <= r^2                                      (h = 0)
//   kind 1 + a  cylinder along axis a: c_a <= v_a < c_a + h, and the squared distance over the other two axes <= r^2   (h >= 1)
//
// Every row (y, z) of a shape holds an interval of x: [cx - w, cx + w] with w = isqrt(r^2 - what the row's y and z use up), or the
// whole [cx, cx + h) of a cylinder along x.  The intervals of all rows are nested around the same centre, so the union over any
// set of rows is the interval of the row nearest to the axis -- which is how a brick row's bricks come out without a loop.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VRC_SHAPE_FN __host__ __device__ inline
#else
#define VRC_SHAPE_FN inline
#endif

namespace vrc {

constexpr int32_t kShapeBall = 0, kShapeCylinderX = 1, kShapeKinds = 4;    // (vrc.h's VRC_SHAPE_*; cylinder along axis a: 1 + a)
constexpr int32_t kShapeMaxRadius = 1 << 30;

struct ShapeOp { int32_t kind, c[3], r, h; };            // one operation as the caller's six integers
struct ShapeSpan { int64_t a, b; };                      // [a, b); empty when a >= b

// floor(sqrt(v)) for 0 <= v <= 2^61.  The double root of a 61-bit v is within 1e-6 of the real one, so the truncated root is off by
// at most one in either direction -- and it IS off near k^2 for k around 2^30, where v has more bits than a double's mantissa:
// one step down and one step up, decided by integer products ((s + 1)^2 < 2^62), make it exact.
VRC_SHAPE_FN int64_t isqrt64(int64_t v) {
    int64_t s = (int64_t)sqrt((double)v);
    s -= s * s > v ? 1 : 0;
    s += (s + 1) * (s + 1) <= v ? 1 : 0;
    return s;
}

// what the _device call skips and the host call refuses
VRC_SHAPE_FN bool shape_valid(const ShapeOp &s, int32_t material) {
    return s.kind >= 0 && s.kind < kShapeKinds && s.r >= 0 && s.r <= kShapeMaxRadius && (s.kind == kShapeBall ? s.h == 0 : s.h >= 1)
           && material >= -128 && material <= 127;
}

// the extent [lo, hi) of the shape along axis k, in 64 bits (c + h and c + r never wrap)
VRC_SHAPE_FN ShapeSpan shape_extent(const ShapeOp &s, int k) {
    const int64_t c = s.c[k];
    if (s.kind == kShapeCylinderX + k) return {c, c + (int64_t)s.h};
    return {c - (int64_t)s.r, c + (int64_t)s.r + 1};
}

// the x interval of the shape on row (y, z)
VRC_SHAPE_FN ShapeSpan shape_row_span(const ShapeOp &s, int64_t y, int64_t z) {
    const int64_t r = s.r;
    int64_t t = r * r;                                   // what is left of r^2 for x
    bool in = true;
    for (int k = 1; k < 3; k++) {
        const int64_t d = (k == 1 ? y : z) - (int64_t)s.c[k];
        if (s.kind == kShapeCylinderX + k) {
            in = in && d >= 0 && d < (int64_t)s.h;
        } else {
            const int64_t ad = d < 0 ? -d : d, q = ad <= r ? ad : 0;      // (|d| > r: outside before anything is squared)
            in = in && ad <= r;
            t -= q * q;
        }
    }
    if (!in || t < 0) return {0, 0};
    const int64_t cx = s.c[0];
    if (s.kind == kShapeCylinderX) return {cx, cx + (int64_t)s.h};
    const int64_t w = isqrt64(t);
    return {cx - w, cx + w + 1};
}

// The bricks [a, b) of brick row (by, bz) -- bricks of 1 << log2 voxels, map-aligned -- that hold a voxel of the shape inside the
// scene [0, lim): the span of the row nearest to the axis among the brick row's in-scene rows, clipped and shifted.  Along a
// cylinder's own axis every row of [c, c + h) has the same span, so any row of the intersection will do.
VRC_SHAPE_FN ShapeSpan shape_brick_row(const ShapeOp &s, int64_t by, int64_t bz, const int32_t lim[3], int log2) {
    int64_t at[3] = {0, 0, 0};
    for (int k = 1; k < 3; k++) {
        const int64_t b = k == 1 ? by : bz;
        int64_t lo = b << log2, hi = (b + 1) << log2;
        if (hi > lim[k]) hi = lim[k];
        if (s.kind == kShapeCylinderX + k) {
            const ShapeSpan e = shape_extent(s, k);
            if (e.a > lo) lo = e.a;
            if (e.b < hi) hi = e.b;
        }
        if (lo >= hi) return {0, 0};
        const int64_t c = s.c[k];
        at[k] = c < lo ? lo : (c > hi - 1 ? hi - 1 : c);
    }
    ShapeSpan x = shape_row_span(s, at[1], at[2]);
    if (x.a < 0) x.a = 0;
    if (x.b > lim[0]) x.b = lim[0];
    if (x.a >= x.b) return {0, 0};
    return {x.a >> log2, ((x.b - 1) >> log2) + 1};
}

}  // namespace vrc
