// Device code shared by the training-input kernels (augment.hip, gt_sample.hip): the reference's BEV corners and box_collision_test,
// the face planes of points_in_rbbox, and the counter-based generator with its keyed bijection.  Every expression follows the
// reference's float32 order (the library builds with -ffp-contract=off); both files must give the same bits for the same box.
#pragma once
#include "pp_common.h"

namespace {

// corners_norm of box2d_to_corner_jit / center_to_corner_box2d: (-.5,-.5) (-.5,.5) (.5,.5) (.5,-.5)
__device__ __constant__ float NX[4] = {-0.5f, -0.5f, 0.5f, 0.5f};
__device__ __constant__ float NY[4] = {-0.5f, 0.5f, 0.5f, -0.5f};

// box2d_to_corner_jit (box_np_ops.py:659-679) of one (x, y, l, w, r): (dims * norm) @ [[c, s], [-s, c]] + xy, float32
__device__ __forceinline__ void bev_corners(float x, float y, float l, float w, float r, float* c)
{
    const float s = sinf(r), co = cosf(r);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float cx = l * NX[k], cy = w * NY[k];
        c[2 * k] = (cx * co + cy * (-s)) + x;
        c[2 * k + 1] = (cx * s + cy * co) + y;
    }
}

// corner_to_standup_nd_jit: xmin, ymin, xmax, ymax
__device__ __forceinline__ void standup(const float* c, float* s)
{
    s[0] = fminf(fminf(c[0], c[2]), fminf(c[4], c[6]));
    s[1] = fminf(fminf(c[1], c[3]), fminf(c[5], c[7]));
    s[2] = fmaxf(fmaxf(c[0], c[2]), fmaxf(c[4], c[6]));
    s[3] = fmaxf(fmaxf(c[1], c[3]), fmaxf(c[5], c[7]));
}

// every corner of q strictly inside the clockwise box b (:661-676; vec = -(b[k] - b[k+1]))
__device__ __forceinline__ bool inside_all(const float* b, const float* q)
{
    for (int l = 0; l < 4; ++l)
        for (int k = 0; k < 4; ++k) {
            const int k1 = (k + 1) & 3;
            const float v0 = -(b[2 * k] - b[2 * k1]), v1 = -(b[2 * k + 1] - b[2 * k1 + 1]);
            float cross = v1 * (b[2 * k] - q[2 * l]);
            cross -= v0 * (b[2 * k + 1] - q[2 * l + 1]);
            if (cross >= 0.f) return false;
        }
    return true;
}

// box_collision_test (:617-697) of one pair.  `ret[i, j] is True / is False` are value tests under numba (the deployed reference):
// without an edge crossing, containment either way is a collision.
__device__ bool collide(const float* b, const float* bs, const float* q, const float* qs)
{
    const float iw = fminf(bs[2], qs[2]) - fmaxf(bs[0], qs[0]);
    if (!(iw > 0.f)) return false;
    const float ih = fminf(bs[3], qs[3]) - fmaxf(bs[1], qs[1]);
    if (!(ih > 0.f)) return false;
    for (int k = 0; k < 4; ++k) {
        const float A0 = b[2 * k], A1 = b[2 * k + 1], B0 = b[2 * ((k + 1) & 3)], B1 = b[2 * ((k + 1) & 3) + 1];
        for (int l = 0; l < 4; ++l) {
            const float C0 = q[2 * l], C1 = q[2 * l + 1], D0 = q[2 * ((l + 1) & 3)], D1 = q[2 * ((l + 1) & 3) + 1];
            const bool acd = (D1 - A1) * (C0 - A0) > (C1 - A1) * (D0 - A0);
            const bool bcd = (D1 - B1) * (C0 - B0) > (C1 - B1) * (D0 - B0);
            if (acd != bcd) {
                const bool abc = (C1 - A1) * (B0 - A0) > (B1 - A1) * (C0 - A0);
                const bool abd = (D1 - A1) * (B0 - A0) > (B1 - A1) * (D0 - A0);
                if (abc != abd) return true;
            }
        }
    }
    return inside_all(b, q) || inside_all(q, b);
}

// prefilter slack of the membership test: 8 mm at 80 m.  The face-plane sign of a point at distance d outside a face is ~|n| d, its
// float32 rounding a few ulp of |n| |p|: below 1e-4 (1 + |p|) for every box that fits the capacity, so the prefilter never rejects
// a point the plane test would keep
constexpr float AABB_PAD = 1e-4f;

// points_in_rbbox's planes of one box (x, y, z, l, w, h, r), origin (0.5, 0.5, 0.5): pl[6] = (normal, -d), bb[6] = the padded AABB
// of the 8 corners (lo xyz, hi xyz)
__device__ __forceinline__ void box_face_planes(const float* b, float4* pl, float* bb)
{
    // center_to_corner_box3d(origin (0.5, 0.5, 0.5), axis 2): corners_nd order, rotation_3d_in_axis's einsum, + centre
    const float s = sinf(b[6]), co = cosf(b[6]);
    float cx[8], cy[8], cz[8];
    const int ux[8] = {0, 0, 0, 0, 1, 1, 1, 1}, uy[8] = {0, 0, 1, 1, 0, 0, 1, 1}, uz[8] = {0, 1, 1, 0, 0, 1, 1, 0};
    float lo[3] = {3.4e38f, 3.4e38f, 3.4e38f}, hi[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
    for (int q = 0; q < 8; ++q) {
        const float dx = b[3] * ((float)ux[q] - 0.5f), dy = b[4] * ((float)uy[q] - 0.5f), dz = b[5] * ((float)uz[q] - 0.5f);
        cx[q] = (dx * co + dy * (-s)) + b[0];
        cy[q] = (dx * s + dy * co) + b[1];
        cz[q] = dz + b[2];
        lo[0] = fminf(lo[0], cx[q]); hi[0] = fmaxf(hi[0], cx[q]);
        lo[1] = fminf(lo[1], cy[q]); hi[1] = fmaxf(hi[1], cy[q]);
        lo[2] = fminf(lo[2], cz[q]); hi[2] = fmaxf(hi[2], cz[q]);
    }
    // corner_to_surfaces_3d_jit + surface_equ_3d_jit: n = (P0 - P1) x (P1 - P2), d = n . P0
    const int sf[6][3] = {{0, 1, 2}, {7, 6, 5}, {0, 3, 7}, {1, 5, 6}, {0, 4, 5}, {3, 2, 6}};
    for (int q = 0; q < 6; ++q) {
        const int i0 = sf[q][0], i1 = sf[q][1], i2 = sf[q][2];
        const float ax = cx[i0] - cx[i1], ay = cy[i0] - cy[i1], az = cz[i0] - cz[i1];
        const float bx = cx[i1] - cx[i2], by = cy[i1] - cy[i2], bz = cz[i1] - cz[i2];
        const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        const float d = (nx * cx[i0] + ny * cy[i0]) + nz * cz[i0];
        pl[q] = make_float4(nx, ny, nz, -d);
    }
    for (int q = 0; q < 3; ++q) {
        bb[q] = lo[q] - AABB_PAD * (1.f + fabsf(lo[q]));
        bb[3 + q] = hi[q] + AABB_PAD * (1.f + fabsf(hi[q]));
    }
}

// the membership decision of points_in_rbbox for one point: inside at sign < 0 on all six faces (outside at sign >= 0)
__device__ __forceinline__ bool inside_box(float x, float y, float z, const float4* pl, const float* bb)
{
    if (x < bb[0] || x > bb[3] || y < bb[1] || y > bb[4] || z < bb[2] || z > bb[5]) return false;
    bool in = true;
    for (int h = 0; h < 6 && in; ++h) {
        const float4 a = pl[h];
        const float sgn = ((x * a.x + y * a.y) + z * a.z) + a.w;
        in = sgn < 0.f;
    }
    return in;
}

// ---- device random mode ------------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11), key = the 64-bit seed, counter = (element, stream | epoch << 8, sample index lo, hi):
// a frame's draws depend only on (seed, epoch, sample index), never on the batch it runs in.  Stream ids 0 .. 9 belong to
// pp_augment_draw, PP_GT_STREAM to pp_gt_draw.
struct u32x4 {
    uint32_t x, y, z, w;
};
__device__ __forceinline__ u32x4 philox(u32x4 c, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        c = u32x4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}
constexpr uint32_t PP_GT_STREAM = 16u;

// keyed bijection of [0, n): a balanced Feistel network of FEISTEL_ROUNDS rounds on 2h >= ceil(log2 n) bits, cycle-walked back
// into [0, n) (at most 4 steps expected)
constexpr int FEISTEL_ROUNDS = 8;
__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t feistel_keyed(uint32_t k, uint32_t n, uint32_t k0, uint32_t k1)
{
    if (n <= 1) return k;
    int bits = 32 - __clz(n - 1);
    const int h = (bits + 1) >> 1;
    const uint32_t mask = (1u << h) - 1u;
    uint32_t x = k;
    do {
        uint32_t L = x >> h, R = x & mask;
        for (int r = 0; r < FEISTEL_ROUNDS; ++r) {
            const uint32_t F = mix32(R ^ (r & 1 ? k1 : k0) ^ (uint32_t)r * 0x9E3779B9u) & mask;
            const uint32_t nl = R;
            R = L ^ F;
            L = nl;
        }
        x = (L << h) | R;
    } while (x >= n);
    return x;
}

} // namespace
