// shape_span_check.cpp -- csrc/shape_span.hpp on the host, built by tests/test_shape_fills_cpu.py with g++ under AddressSanitizer
// and UBSan (a signed overflow in the span arithmetic is an error, not a wrap):
//   1. isqrt64 against its definition (s >= 0, s^2 <= v < (s + 1)^2) for every v < 2^20, for k^2 - 1, k^2, k^2 + 1 with every k
//      of [2^30 - 4096, 2^30] and with a few thousand k spread over (2^26, 2^30); how often the bare (int64_t)sqrt((double)v)
//      is wrong on those inputs is counted and printed
//   2. shape_row_span against per-voxel membership, written out here a second time, over a 20 x 12 x 17 scene: shapes of all four
//      kinds with r <= 12, h <= 10 and centres in [-4, 24)^3 drawn by a fixed generator, and the extreme ones of the contract
//   3. shape_brick_row against the brick set those voxels give by brute force: that scene with bricks of 8, 4 and 2, and the
//      scenes of the shallow trees (dim 2 and 4: the brick is the scene) with their own brick and with the 8^3 one the kernels use
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "shape_span.hpp"

namespace {

constexpr int DX = 20, DY = 12, DZ = 17;
long long g_roots = 0, g_bare_wrong = 0, g_shapes = 0, g_rows = 0, g_brick_rows = 0;

int fail(const char *what, long long a, long long b, long long c) {
    printf("FAILED %s: %lld %lld %lld\n", what, a, b, c);
    return 1;
}

int check_root(int64_t v) {
    const int64_t s = vrc::isqrt64(v);
    g_roots++;
    if ((int64_t)sqrt((double)v) != s) g_bare_wrong++;
    if (s < 0 || s * s > v || (s + 1) * (s + 1) <= v) return fail("isqrt64", v, s, 0);
    return 0;
}

int check_around(int64_t k) {
    return check_root(k * k - 1) || check_root(k * k) || check_root(k * k + 1);
}

// the contract's membership, voxel by voxel
bool member(const vrc::ShapeOp &s, int64_t x, int64_t y, int64_t z) {
    const int64_t v[3] = {x, y, z}, r = s.r;
    int64_t sum = 0;
    for (int a = 0; a < 3; a++) {
        const int64_t d = v[a] - (int64_t)s.c[a];
        if (s.kind == 1 + a) {
            if (d < 0 || d >= (int64_t)s.h) return false;
        } else {
            if (d > r || -d > r) return false;                   // (first: d^2 is at most 2^60 from here on)
            sum += d * d;
        }
    }
    return sum <= r * r;
}

int check_bricks(const vrc::ShapeOp &s, const std::vector<uint8_t> &in, int dx, int dy, int dz, int log2) {
    const int32_t lim[3] = {dx, dy, dz};
    const int side = 1 << log2, nbx = (dx + side - 1) >> log2, nby = (dy + side - 1) >> log2, nbz = (dz + side - 1) >> log2;
    for (int bz = 0; bz < nbz; bz++)
        for (int by = 0; by < nby; by++) {
            std::vector<uint8_t> touched((size_t)nbx, 0);
            for (int z = bz << log2; z < ((bz + 1) << log2) && z < dz; z++)
                for (int y = by << log2; y < ((by + 1) << log2) && y < dy; y++)
                    for (int x = 0; x < dx; x++)
                        if (in[(size_t)x + DX * ((size_t)y + DY * (size_t)z)]) touched[(size_t)(x >> log2)] = 1;
            const vrc::ShapeSpan b = vrc::shape_brick_row(s, by, bz, lim, log2);
            g_brick_rows++;
            if (b.a < b.b && (b.a < 0 || b.b > nbx)) return fail("brick interval outside the scene", b.a, b.b, log2);
            for (int bx = 0; bx < nbx; bx++)
                if ((touched[(size_t)bx] != 0) != (bx >= b.a && bx < b.b)) return fail("shape_brick_row", s.kind, by * 1000 + bz, bx * 10 + log2);
        }
    return 0;
}

int check_shape(const vrc::ShapeOp &s) {
    if (!vrc::shape_valid(s, 0)) return fail("the check's own shape is invalid", s.kind, s.r, s.h);
    g_shapes++;
    std::vector<uint8_t> in((size_t)DX * DY * DZ, 0);
    for (int z = 0; z < DZ; z++)
        for (int y = 0; y < DY; y++) {
            const vrc::ShapeSpan span = vrc::shape_row_span(s, y, z);
            g_rows++;
            for (int x = 0; x < DX; x++) {
                const bool want = member(s, x, y, z);
                in[(size_t)x + DX * ((size_t)y + DY * (size_t)z)] = want;
                if (want != (span.a < span.b && x >= span.a && x < span.b)) return fail("shape_row_span", s.kind, x, y * 100 + z);
            }
            // beside the scene too: the span is the row's, not the scene's
            for (int64_t x : {(int64_t)-9, (int64_t)-1, (int64_t)DX, (int64_t)DX + 7, span.a - 1, span.a, span.b - 1, span.b})
                if (member(s, x, y, z) != (span.a < span.b && x >= span.a && x < span.b)) return fail("shape_row_span beside the scene", s.kind, x, y * 100 + z);
        }
    for (int log2 = 1; log2 <= 3; log2++)
        if (check_bricks(s, in, DX, DY, DZ, log2)) return 1;
    return check_bricks(s, in, 2, 2, 2, 1) || check_bricks(s, in, 2, 2, 2, 3) || check_bricks(s, in, 4, 4, 4, 2) || check_bricks(s, in, 4, 4, 4, 3);
}

}  // namespace

int main() {
    for (int64_t v = 0; v < (1 << 20); v++)
        if (check_root(v)) return 1;
    for (int64_t k = (1LL << 30) - 4096; k <= (1LL << 30); k++)
        if (check_around(k)) return 1;
    for (int64_t i = 0; i < 4000; i++)
        if (check_around((1LL << 26) + 3 + i * 241807)) return 1;                 // (the last one: 2^26 + 967 million < 2^30)
    for (int64_t k : {(1LL << 30) - 1, (1LL << 27) + 1, 94906267LL, (1LL << 26) + 3})
        if (check_around(k)) return 1;
    if (check_root(1LL << 61) || check_root((1LL << 61) - 1)) return 1;
    if (g_bare_wrong == 0) return fail("the bare truncated root was never wrong: the inputs do not reach the fix-up", 0, 0, 0);

    // valid and invalid operations
    const vrc::ShapeOp ball{0, {1, 2, 3}, 4, 0}, pipe{2, {1, 2, 3}, 4, 1};
    vrc::ShapeOp bad[6] = {ball, ball, ball, ball, pipe, ball};
    bad[0].kind = 4; bad[1].r = -1; bad[2].r = (1 << 30) + 1; bad[3].h = 1; bad[4].h = 0; bad[5].kind = -1;
    for (const vrc::ShapeOp &s : bad)
        if (vrc::shape_valid(s, 5)) return fail("shape_valid accepts", s.kind, s.r, s.h);
    if (!vrc::shape_valid(ball, -128) || !vrc::shape_valid(pipe, 127) || vrc::shape_valid(ball, 128) || vrc::shape_valid(pipe, -129)) return fail("shape_valid: materials", 0, 0, 0);

    // the small family, drawn by a fixed generator
    uint64_t state = 0x9e3779b97f4a7c15ULL;
    auto draw = [&](int n) { state = state * 6364136223846793005ULL + 1442695040888963407ULL; return (int)((state >> 33) % (uint64_t)n); };
    for (int i = 0; i < 12000; i++) {
        vrc::ShapeOp s;
        s.kind = i & 3;
        for (int a = 0; a < 3; a++) s.c[a] = draw(28) - 4;
        s.r = draw(13);
        s.h = s.kind == 0 ? 0 : 1 + draw(10);
        if (check_shape(s)) return 1;
    }
    // every r and every kind around one brick corner, where the spans cross brick borders one voxel at a time
    for (int kind = 0; kind < 4; kind++)
        for (int r = 0; r <= 12; r++)
            for (int c = 6; c <= 9; c++)
                if (check_shape(vrc::ShapeOp{kind, {c, 8, c == 7 ? 7 : 8}, r, kind == 0 ? 0 : 3})) return 1;
    // the contract's extremes
    const int32_t kMin = INT32_MIN, kMax = INT32_MAX, kR = 1 << 30;
    const vrc::ShapeOp extremes[] = {
        {0, {-kR + 3, 4, 4}, kR, 0},                             // a thin cap at x <= 3
        {0, {4, -kR + 3, 4}, kR, 0}, {0, {4, 4, -kR + 2}, kR, 0},
        {0, {kMin, kMin, kMin}, kR, 0}, {0, {kMax, kMax, kMax}, kR, 0}, {0, {kMax, 5, 5}, kR, 0},
        {1, {kMax - 1, 5, 5}, 7, kMax}, {2, {5, kMax - 1, 5}, 7, kMax}, {3, {5, 5, kMax - 1}, 7, kMax},
        {1, {kMin, 5, 5}, 3, kMax}, {2, {5, kMin, 5}, 3, kMax}, {3, {5, 5, kMin}, 3, kMax},
        {1, {kMin + 2, 5, 5}, 3, kMax}, {2, {5, kMin + 2, 5}, 3, kMax}, {3, {5, 5, kMin + 2}, 3, kMax},
        {1, {-5, kMax, kMin}, kR, kMax}, {2, {kMin, -5, kMax}, kR, kMax}, {3, {kMax, kMin, -5}, kR, kMax},
        {3, {9, 9, 0}, 0, DZ}, {1, {3, 3, 3}, kR, 9}, {2, {-kR, 3, 7}, kR, 4}, {3, {7, kR + 11, 2}, kR, 40},
    };
    for (const vrc::ShapeOp &s : extremes)
        if (check_shape(s)) return 1;
    printf("shape_span ok: roots %lld, bare truncation wrong %lld, shapes %lld, rows %lld, brick rows %lld\n", g_roots, g_bare_wrong, g_shapes, g_rows, g_brick_rows);
    return 0;
}
