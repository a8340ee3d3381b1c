// Training-input augmentation: the part of GenericDataset.__getitem__ (framework/dataset.py:121-146 of the reference) in front of
// voxelisation, batched over nb frames with CSR offsets for boxes and points.
//   N1  noise selection (augmentation.py:122-175 noise_per_box_v2_ + :617-697 box_collision_test): one workgroup per frame, the
//       boxes in order (box i is tested against the boxes already moved), the tries of one box over the lanes, the lowest
//       non-colliding try wins.  The frame's current BEV corners live in LDS.
// prm[PP_AUG_ON] holds step bits (ST_* below): the dataset runs every step, the reference-named functions one each.
//   B1  boxes, one thread per box: box3d_transform_ (:419-425), flip, pitch / roll / yaw (centre only; yaw also adds to r),
//       global_scaling_v2, global_translate, the range filter (box_np_ops.py:6-16) and limit_period(r, 0.5, 2 pi); kept boxes are
//       compacted in order inside the frame's slot.
//   D1  device random mode: the same parameter arrays from Philox4x32-10 keyed by (seed, epoch, sample index); the shuffle is a
//       keyed Feistel bijection evaluated inline by P1 (no permutation array).
//   P1  points, one thread per output row k with src = perm[k]: the first VALID box containing the source point among the
//       ORIGINAL boxes (points_in_rbbox, box_np_ops.py:460-467, origin (0.5, 0.5, 0.5)), that box's move (points_transform_
//       :400-416), then the global chain.  Face planes are built once per block in LDS.
// Every expression follows the reference's float32 / float64 order and dtype (the library builds with -ffp-contract=off).  numpy
// computes `float32_array (op)= float64_array` in float64 and rounds the result to float32: written below as (float)((double)a op b).
// A Python float meeting a float32 array is cast to float32 first (NEP 50, weak scalars): written as (float)x.
#include <cstring>
#include "pp_common.h"
#include "aug_geom.h"

namespace {

constexpr int AUG_GROUP = 64;          // frames per launch (kernel-argument table)
constexpr int MAXB = PP_AUG_MAX_BOXES; // boxes per frame (LDS of N1 and P1)
constexpr int NOISE_THREADS = 128;     // >= PP_AUG_MAX_TRIES: one try per lane
constexpr int BOX_THREADS = MAXB;
constexpr int PTS_THREADS = 256;
constexpr int PTS_PER_THREAD = 4;
constexpr float TWO_PI_F = 6.28318530717958647692f; // 2 * np.pi as a weak Python float against a float32 array
static_assert(NOISE_THREADS >= PP_AUG_MAX_TRIES && NOISE_THREADS % 64 == 0, "k_noise: one lane per try");
static_assert(BOX_THREADS == MAXB && BOX_THREADS % 64 == 0, "k_boxes: one thread per box");
static_assert(MAXB <= PTS_THREADS && PTS_THREADS == 256 && MAXB <= 32767, "k_points: one thread per box for the LDS setup, 4 waves, int16 list");

struct aug_args {
    int32_t boff[AUG_GROUP + 1]; // box rows of the group's frames: frame z owns boff[z] .. boff[z+1]-1
    int32_t poff[AUG_GROUP + 1]; // point rows likewise
    int32_t f0;                  // first frame of the group (frame-strided arrays: prm, kept)
    int32_t T;                   // tries per box
    float range[4];              // x0, y0, x1, y1 of the range filter (float32, as detection_range[[0, 1, 3, 4]])
};

__global__ void __launch_bounds__(NOISE_THREADS) k_noise(aug_args p, const float* __restrict__ boxes, const uint8_t* __restrict__ valid,
                                                         const double* __restrict__ loc, const double* __restrict__ rot,
                                                         const double* __restrict__ grot, int32_t* __restrict__ sel,
                                                         double* __restrict__ sel_loc, double* __restrict__ sel_rot)
{
    __shared__ float cn[MAXB][8];
    __shared__ float sd[MAXB][4];
    __shared__ uint64_t bal[NOISE_THREADS / 64];
    const int z = blockIdx.x, t = threadIdx.x, T = p.T;
    const int b0 = p.boff[z], nbx = p.boff[z + 1] - b0;
    for (int i = t; i < nbx; i += NOISE_THREADS) {
        const float* bx = boxes + (size_t)(b0 + i) * 7;
        bev_corners(bx[0], bx[1], bx[3], bx[4], bx[6], cn[i]);
        standup(cn[i], sd[i]);
    }
    __syncthreads();
    for (int i = 0; i < nbx; ++i) {
        const int g = b0 + i;
        if (!valid[g]) { // not moved, still an obstacle
            if (t == 0) {
                sel[g] = -1;
                sel_loc[3 * g] = sel_loc[3 * g + 1] = sel_loc[3 * g + 2] = 0.0;
                sel_rot[g] = 0.0;
            }
            continue;
        }
        const float* bx = boxes + (size_t)g * 7;
        bool ok = false;
        float c[8], s4[4], dpx = 0.f, dpy = 0.f, cgrot = 0.f;
        double dgrot = 0.0;
        if (t < T) {
            const size_t j = (size_t)g * T + t;
            const float x = bx[0], y = bx[1], l = bx[3], w = bx[4], r = bx[6];
            const float rad = sqrtf(x * x + y * y);      // float32 scalars: boxes[i, 0]**2 + boxes[i, 1]**2
            cgrot = atan2f(y, x);                         // float32
            const double gn = grot[j];
            dgrot = (double)cgrot + gn;                   // float32 + float64 -> float64
            dpx = (float)((double)rad * cos(dgrot));      // float64 product stored into the float32 dst_pos
            dpy = (float)((double)rad * sin(dgrot));
            const float cr = (float)((double)r + gn);     // current_box[0, -1] += grot: float64 sum stored as float32
            const float rs = sinf(cr), rc = cosf(cr);     // float32 rot_mat_T
            const double rn = rot[j];
            const float ns = (float)sin(rn), nc = (float)cos(rn); // _rotation_box2d_jit_: float64 sin / cos into the float32 matrix
            const double ox = (double)dpx + loc[3 * j], oy = (double)dpy + loc[3 * j + 1]; // current_box[0, :2] + loc[:2]: float64
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float cx = l * NX[k], cy = w * NY[k];
                const float x1 = cx * rc + cy * (-rs), y1 = cx * rs + cy * rc;
                const float x2 = x1 * nc + y1 * (-ns), y2 = x1 * ns + y1 * nc;
                c[2 * k] = (float)((double)x2 + ox); // float32 corners += float64 vector
                c[2 * k + 1] = (float)((double)y2 + oy);
            }
            standup(c, s4);
            ok = true;
            for (int k = 0; k < nbx; ++k) {
                if (k == i) continue; // coll_mat[0, i] = False
                if (collide(c, s4, cn[k], sd[k])) {
                    ok = false;
                    break;
                }
            }
        }
        const uint64_t m = __ballot(ok);
        if ((t & 63) == 0) bal[t >> 6] = m;
        __syncthreads();
        int win = -1;
#pragma unroll
        for (int q = NOISE_THREADS / 64 - 1; q >= 0; --q)
            if (bal[q]) win = 64 * q + __ffsll((unsigned long long)bal[q]) - 1;
        if (t == win) {
#pragma unroll
            for (int k = 0; k < 8; ++k) cn[i][k] = c[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) sd[i][k] = s4[k];
            const size_t j = (size_t)g * T + t;
            sel[g] = win;
            sel_loc[3 * g] = loc[3 * j] + (double)(dpx - bx[0]);     // loc[:2] += (dst_pos - boxes[i, :2]): float32 difference
            sel_loc[3 * g + 1] = loc[3 * j + 1] + (double)(dpy - bx[1]);
            sel_loc[3 * g + 2] = loc[3 * j + 2];
            sel_rot[g] = rot[j] + (dgrot - (double)cgrot);           // rot += (dst_grot - current_grot): float64
        } else if (win < 0 && t == 0) {
            sel[g] = -1;
            sel_loc[3 * g] = sel_loc[3 * g + 1] = sel_loc[3 * g + 2] = 0.0;
            sel_rot[g] = 0.0;
        }
        __syncthreads();
    }
}

// float32 rotation matrix of rotation_points_single_angle (box_np_ops.py:629-648): built from float64 sin / cos
struct rot3 {
    float c, s;
};
__device__ __forceinline__ rot3 mk_rot(double a) { return rot3{(float)cos(a), (float)sin(a)}; }

// step bits of prm[PP_AUG_ON]: the dataset runs all of them, the reference-named single functions one each
constexpr int ST_MOVE = 1, ST_FLIP = 2, ST_ROT = 4, ST_SCALE = 8, ST_TRANS = 16, ST_RANGE = 32, ST_PERM = 64;

// random_flip + global_rotation_v2 on one float32 xyz: p @ rot_mat_T with the zero terms dropped (adding +-0 to a float32 sum
// changes nothing but the sign of an exact zero)
__device__ __forceinline__ void global_rotate(float& x, float& y, float& z, int st, bool flip, rot3 pi, rot3 ro, rot3 ya)
{
    if ((st & ST_FLIP) && flip) y = -y;
    if (!(st & ST_ROT)) return;
    { // pitch, axis 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        const float nx = x * pi.c + z * (-pi.s), nz = x * pi.s + z * pi.c;
        x = nx; z = nz;
    }
    { // roll, axis 0: [[1, 0, 0], [0, c, -s], [0, s, c]]
        const float ny = y * ro.c + z * ro.s, nz = y * (-ro.s) + z * ro.c;
        y = ny; z = nz;
    }
    { // yaw, axis 2: [[c, s, 0], [-s, c, 0], [0, 0, 1]]
        const float nx = x * ya.c + y * (-ya.s), ny = x * ya.s + y * ya.c;
        x = nx; y = ny;
    }
}

// global_scaling_v2's `[:, :3] *= float64 scales`, then global_translate's `+= float64 noise_translate`
__device__ __forceinline__ void scale_translate(float* v, int st, const double* P)
{
    if (st & ST_SCALE)
        for (int q = 0; q < 3; ++q) v[q] = (float)((double)v[q] * P[PP_AUG_SX + q]);
    if (st & ST_TRANS)
        for (int q = 0; q < 3; ++q) v[q] = (float)((double)v[q] + P[PP_AUG_TX + q]);
}

// filter_gt_box_outside_range with kitti_io.gt_in_range's semantics: some BEV corner strictly inside the clockwise range rectangle
__device__ __forceinline__ bool in_range(const float* b, const float* rg)
{
    const float poly[8] = {rg[0], rg[1], rg[0], rg[3], rg[2], rg[3], rg[2], rg[1]};
    const float s = sinf(b[6]), co = cosf(b[6]);
    bool any = false;
    for (int q = 0; q < 4; ++q) {
        const float cx = b[3] * NX[q], cy = b[4] * NY[q];
        const float px = (cx * co + cy * (-s)) + b[0], py = (cx * s + cy * co) + b[1];
        bool in = true;
        for (int k = 0; k < 4; ++k) {
            const int km = (k + 3) & 3;
            const float v0 = poly[2 * k] - poly[2 * km], v1 = poly[2 * k + 1] - poly[2 * km + 1];
            const float cross = v1 * (poly[2 * k] - px) - v0 * (poly[2 * k + 1] - py);
            in = in && cross < 0.f;
        }
        any = any || in;
    }
    return any;
}

__global__ void __launch_bounds__(BOX_THREADS) k_boxes(aug_args p, const float* __restrict__ boxes, const int32_t* __restrict__ cls,
                                                       const uint8_t* __restrict__ valid, const double* __restrict__ sel_loc,
                                                       const double* __restrict__ sel_rot, const double* __restrict__ prm,
                                                       float* __restrict__ out, int32_t* __restrict__ out_cls, uint8_t* __restrict__ keep,
                                                       int32_t* __restrict__ kept)
{
    __shared__ int wcnt[BOX_THREADS / 64];
    const int z = blockIdx.x, i = threadIdx.x, f = p.f0 + z;
    const int b0 = p.boff[z], n = p.boff[z + 1] - b0, g = b0 + i;
    const double* P = prm + (size_t)f * PP_AUG_PARAMS;
    float b[7] = {};
    bool k = false;
    if (i < n) {
#pragma unroll
        for (int q = 0; q < 7; ++q) b[q] = boxes[(size_t)g * 7 + q];
        const int st = (int)P[PP_AUG_ON];
        if ((st & ST_MOVE) && valid[g]) { // box3d_transform_: float32 += float64
            for (int q = 0; q < 3; ++q) b[q] = (float)((double)b[q] + sel_loc[3 * g + q]);
            b[6] = (float)((double)b[6] + sel_rot[g]);
        }
        const bool flip = P[PP_AUG_FLIP] != 0.0;
        if ((st & ST_FLIP) && flip) b[6] = -b[6];
        global_rotate(b[0], b[1], b[2], st, flip, mk_rot(P[PP_AUG_PITCH]), mk_rot(P[PP_AUG_ROLL]), mk_rot(P[PP_AUG_YAW]));
        if (st & ST_ROT) b[6] = b[6] + (float)P[PP_AUG_YAW]; // gt_boxes[:, 6] += yaw (weak Python float)
        if (st & ST_SCALE) {
            for (int q = 0; q < 3; ++q) b[q] = (float)((double)b[q] * P[PP_AUG_SX + q]);
            const float fx = (float)P[PP_AUG_SX], fy = (float)P[PP_AUG_SY]; // x_scale * float32 array: weak -> float32
            const float cr = cosf(b[6]), sr = sinf(b[6]);
            const float a0 = fx * cr, a1 = fy * sr, c0 = fx * sr, c1 = fy * cr;
            b[3] = b[3] * sqrtf(a0 * a0 + a1 * a1);
            b[4] = b[4] * sqrtf(c0 * c0 + c1 * c1);
            b[5] = b[5] * (float)P[PP_AUG_SZ];
            b[6] = atanf(tanf(b[6]) * (float)(P[PP_AUG_SY] / P[PP_AUG_SX])); // r * (y_scale / x_scale): the Python quotient, weak
        }
        if (st & ST_TRANS)
            for (int q = 0; q < 3; ++q) b[q] = (float)((double)b[q] + P[PP_AUG_TX + q]);
        k = true;
        if (st & ST_RANGE) {
            k = in_range(b, p.range);
            b[6] = b[6] - floorf(b[6] / TWO_PI_F + 0.5f) * TWO_PI_F; // limit_period(r, 0.5, 2 pi), float32
        }
        keep[g] = k ? 1 : 0;
    }
    // in-order compaction of the kept boxes inside the frame's slot
    const uint64_t m = __ballot(k);
    const int lane = i & 63, wv = i >> 6;
    if (lane == 0) wcnt[wv] = __popcll(m);
    __syncthreads();
    int base = 0, total = 0;
    for (int q = 0; q < BOX_THREADS / 64; ++q) {
        base += q < wv ? wcnt[q] : 0;
        total += wcnt[q];
    }
    const int rank = base + __popcll(m & ((1ull << lane) - 1ull));
    if (k) {
        for (int q = 0; q < 7; ++q) out[(size_t)(b0 + rank) * 7 + q] = b[q];
        out_cls[b0 + rank] = cls[g];
    }
    if (i >= total && i < n) { // rows behind the kept ones: zero
        for (int q = 0; q < 7; ++q) out[(size_t)g * 7 + q] = 0.f;
        out_cls[g] = 0;
    }
    if (i == 0) kept[f] = total;
}

// ---- device random mode ------------------------------------------------------------------------------------------------------
// Philox4x32-10 and the keyed Feistel bijection: aug_geom.h
// 53-bit uniforms in [0, 1) from two words (numpy's random_standard_uniform construction)
__device__ __forceinline__ double u53(uint32_t a, uint32_t b) { return (double)(((uint64_t)(a >> 5) << 26) | (b >> 6)) * 0x1.0p-53; }
// Box-Muller in float64: (1 - u1) in (0, 1]
__device__ __forceinline__ void box_muller(double u1, double u2, double& z0, double& z1)
{
    const double r = sqrt(-2.0 * log(1.0 - u1)), t = 6.283185307179586 * u2;
    z0 = r * cos(t);
    z1 = r * sin(t);
}

// the permutation's 64-bit key sits in prm[PP_AUG_KEY_LO / _HI] as exact doubles
__device__ __forceinline__ uint32_t feistel(uint32_t k, uint32_t n, const double* P)
{
    return feistel_keyed(k, n, (uint32_t)P[PP_AUG_KEY_LO], (uint32_t)P[PP_AUG_KEY_HI]);
}

struct draw_args {
    int32_t boff[AUG_GROUP + 1];
    int64_t sample[AUG_GROUP];
    int32_t f0, T, steps;
    uint32_t k0, k1, epoch;
};

// the draws of draw_frame from the counter-based generator: loc / rot / grot per (box, try), the frame parameters and the
// permutation key per frame.  One thread per (box, try); thread 0 of block 0 of a frame writes the frame's prm row.
__global__ void __launch_bounds__(256) k_draw(draw_args a, double* __restrict__ loc, double* __restrict__ rot, double* __restrict__ grot,
                                              double* __restrict__ prm)
{
    const int z = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b0 = a.boff[z], ne = (a.boff[z + 1] - b0) * a.T;
    const uint32_t s_lo = (uint32_t)a.sample[z], s_hi = (uint32_t)((uint64_t)a.sample[z] >> 32), ep = a.epoch << 8;
    if (e < ne) {
        const size_t j = (size_t)b0 * a.T + e;
        const u32x4 r0 = philox(u32x4{(uint32_t)e, ep | 0u, s_lo, s_hi}, a.k0, a.k1);
        const u32x4 r1 = philox(u32x4{(uint32_t)e, ep | 1u, s_lo, s_hi}, a.k0, a.k1);
        const u32x4 r2 = philox(u32x4{(uint32_t)e, ep | 2u, s_lo, s_hi}, a.k0, a.k1);
        const double sd = (double)0.15f; // center_noise_std in float32, as noise_per_object builds it
        double n0, n1, n2, n3;
        box_muller(u53(r0.x, r0.y), u53(r0.z, r0.w), n0, n1);
        box_muller(u53(r1.x, r1.y), u53(r1.z, r1.w), n2, n3);
        loc[3 * j] = sd * n0;
        loc[3 * j + 1] = sd * n1;
        loc[3 * j + 2] = sd * n2;
        const double rp = (5.0 / 180) * 3.141592653589793, gp = (2.0 / 180) * 3.141592653589793;
        rot[j] = -rp + 2.0 * rp * u53(r2.x, r2.y);
        grot[j] = -gp + 2.0 * gp * u53(r2.z, r2.w);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double* P = prm + (size_t)(a.f0 + z) * PP_AUG_PARAMS;
        const uint32_t fe = 0xFFFFFFFFu; // frame-level element id
        const u32x4 q0 = philox(u32x4{fe, ep | 3u, s_lo, s_hi}, a.k0, a.k1);
        const u32x4 q1 = philox(u32x4{fe, ep | 4u, s_lo, s_hi}, a.k0, a.k1);
        const u32x4 q2 = philox(u32x4{fe, ep | 5u, s_lo, s_hi}, a.k0, a.k1);
        const u32x4 q3 = philox(u32x4{fe, ep | 6u, s_lo, s_hi}, a.k0, a.k1);
        const u32x4 q4 = philox(u32x4{fe, ep | 7u, s_lo, s_hi}, a.k0, a.k1);
        const u32x4 q5 = philox(u32x4{fe, ep | 9u, s_lo, s_hi}, a.k0, a.k1);
        for (int q = 0; q < PP_AUG_PARAMS; ++q) P[q] = 0.0;
        const bool augm = a.steps & ST_MOVE;
        P[PP_AUG_ON] = (double)a.steps;
        P[PP_AUG_SX] = P[PP_AUG_SY] = P[PP_AUG_SZ] = 1.0;
        if (augm) {
            const double pi = 3.141592653589793;
            P[PP_AUG_FLIP] = u53(q0.x, q0.y) > 0.5 ? 1.0 : 0.0;
            P[PP_AUG_PITCH] = (-4.0 + 8.0 * u53(q0.z, q0.w)) / 180 * pi;
            P[PP_AUG_ROLL] = (-2.0 + 4.0 * u53(q1.x, q1.y)) / 180 * pi;
            P[PP_AUG_YAW] = (-30.0 + 60.0 * u53(q1.z, q1.w)) / 180 * pi;
            P[PP_AUG_SX] = 0.9 + 0.2 * u53(q2.x, q2.y);
            P[PP_AUG_SY] = 0.9 + 0.2 * u53(q2.z, q2.w);
            P[PP_AUG_SZ] = 0.95 + 0.1 * u53(q3.x, q3.y);
            double t0, t1, t2, t3;
            box_muller(u53(q3.z, q3.w), u53(q4.x, q4.y), t0, t1);
            box_muller(u53(q4.z, q4.w), u53(q5.x, q5.y), t2, t3);
            P[PP_AUG_TX] = 0.25 * t0;
            P[PP_AUG_TY] = 0.25 * t1;
            P[PP_AUG_TZ] = 0.25 * t2;
        }
        const u32x4 kq = philox(u32x4{fe, ep | 8u, s_lo, s_hi}, a.k0, a.k1);
        P[PP_AUG_KEY_LO] = (double)kq.x;
        P[PP_AUG_KEY_HI] = (double)kq.y;
    }
}

__global__ void __launch_bounds__(PTS_THREADS) k_points(aug_args p, const float4* __restrict__ pts, const int32_t* __restrict__ perm,
                                                        const float* __restrict__ boxes, const uint8_t* __restrict__ valid,
                                                        const double* __restrict__ sel_loc, const double* __restrict__ sel_rot,
                                                        const double* __restrict__ prm, float4* __restrict__ out)
{
    __shared__ float4 pl[MAXB][6];     // face planes (normal, -d) of the original boxes
    __shared__ float bb[MAXB][6];      // padded AABB of the 8 corners
    __shared__ float ctr[MAXB][4];     // centre; cos, sin of the selected rotation are in mv
    __shared__ float mv[MAXB][2];
    __shared__ double sl[MAXB][3];     // selected loc (float64)
    __shared__ int16_t list[MAXB];     // valid boxes in order
    __shared__ int nvalid;
    __shared__ float gm[6];            // global rotations: pitch c, s, roll c, s, yaw c, s
    const int z = blockIdx.y, f = p.f0 + z, t = threadIdx.x;
    const int p0 = p.poff[z], np_ = p.poff[z + 1] - p0;
    const int64_t first = (int64_t)blockIdx.x * PTS_THREADS * PTS_PER_THREAD;
    if (first >= np_) return; // uniform over the block
    const double* P = prm + (size_t)f * PP_AUG_PARAMS;
    const int st = (int)P[PP_AUG_ON];
    const int b0 = p.boff[z], nbx = (st & ST_MOVE) ? p.boff[z + 1] - b0 : 0;
    bool v = false;
    if (t < nbx) {
        const int g = b0 + t;
        v = valid[g] != 0;
        const float* b = boxes + (size_t)g * 7;
        box_face_planes(b, pl[t], bb[t]);
        ctr[t][0] = b[0]; ctr[t][1] = b[1]; ctr[t][2] = b[2];
        const rot3 r = mk_rot(sel_rot[g]); // _rotation_matrix_3d_: float64 sin / cos into the float32 matrix
        mv[t][0] = r.c; mv[t][1] = r.s;
        for (int q = 0; q < 3; ++q) sl[t][q] = sel_loc[3 * g + q];
    }
    if (t == 0) {
        const rot3 a = mk_rot(P[PP_AUG_PITCH]), b = mk_rot(P[PP_AUG_ROLL]), c = mk_rot(P[PP_AUG_YAW]);
        gm[0] = a.c; gm[1] = a.s; gm[2] = b.c; gm[3] = b.s; gm[4] = c.c; gm[5] = c.s;
    }
    // in-order list of the valid boxes (nbx <= MAXB = PTS_THREADS)
    __shared__ int wcnt[PTS_THREADS / 64];
    const uint64_t m = __ballot(v);
    const int lane = t & 63, wv = t >> 6;
    if (lane == 0) wcnt[wv] = __popcll(m);
    __syncthreads();
    int base = 0;
    for (int q = 0; q < wv; ++q) base += wcnt[q];
    if (v) list[base + __popcll(m & ((1ull << lane) - 1ull))] = (int16_t)t;
    if (t == 0) nvalid = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
    const rot3 pi{gm[0], gm[1]}, ro{gm[2], gm[3]}, ya{gm[4], gm[5]};
    const int nv = nvalid;
    for (int u = 0; u < PTS_PER_THREAD; ++u) {
        const int64_t k = first + (int64_t)u * PTS_THREADS + t;
        if (k >= np_) break;
        int src = (st & ST_PERM) ? (int)feistel((uint32_t)k, (uint32_t)np_, P) : perm ? perm[p0 + k] : (int)k;
        if ((unsigned)src >= (unsigned)np_) src = (int)k; // perm is not validated: a stray entry reads row k, never another frame
        float4 q = pts[p0 + src];
        if (st) {
            float x = q.x, y = q.y, zz = q.z;
            for (int e = 0; e < nv; ++e) {
                const int j = list[e];
                if (!inside_box(x, y, zz, pl[j], bb[j])) continue;
                // points_transform_: -= centre, @ yaw matrix, += centre, += loc (float64)
                const float c = mv[j][0], s = mv[j][1];
                const float px = x - ctr[j][0], py = y - ctr[j][1], pz = zz - ctr[j][2];
                const float rx = px * c + py * (-s), ry = px * s + py * c;
                x = (float)((double)(rx + ctr[j][0]) + sl[j][0]);
                y = (float)((double)(ry + ctr[j][1]) + sl[j][1]);
                zz = (float)((double)(pz + ctr[j][2]) + sl[j][2]);
                break; // only the first box's transform
            }
            global_rotate(x, y, zz, st, P[PP_AUG_FLIP] != 0.0, pi, ro, ya);
            float v3[3] = {x, y, zz};
            scale_translate(v3, st, P);
            q.x = v3[0]; q.y = v3[1]; q.z = v3[2];
        }
        out[p0 + k] = q;
    }
}

// host checks shared by the three entry points; fills the group table of frames [f0, f0 + g)
int check_off(pp_ctx* ctx, const int32_t* off_h, int nb, int64_t cap_total, int per_frame_cap, const char* what)
{
    if (!off_h) return pp_fail(ctx, PP_E_ARG, what);
    if (off_h[0] != 0) return pp_fail(ctx, PP_E_ARG, "augment: offsets must start at 0");
    for (int f = 0; f < nb; ++f) {
        if (off_h[f + 1] < off_h[f]) return pp_fail(ctx, PP_E_ARG, "augment: offsets are not monotone");
        if (per_frame_cap > 0 && off_h[f + 1] - off_h[f] > per_frame_cap)
            return pp_fail(ctx, PP_E_ARG, "augment: more boxes in a frame than PP_AUG_MAX_BOXES");
    }
    if (off_h[nb] > cap_total) return pp_fail(ctx, PP_E_ARG, "augment: more rows than the call's capacity");
    return 0;
}

aug_args make_args(const int32_t* boff_h, const int32_t* poff_h, int f0, int g, int T, const float* range_h)
{
    aug_args a;
    std::memset(&a, 0, sizeof(a));
    a.f0 = f0;
    a.T = T;
    for (int z = 0; z <= g; ++z) {
        a.boff[z] = boff_h[f0 + z];
        a.poff[z] = poff_h ? poff_h[f0 + z] : 0;
    }
    if (range_h)
        for (int q = 0; q < 4; ++q) a.range[q] = range_h[q];
    return a;
}

} // namespace

extern "C" int pp_augment_noise(pp_ctx* ctx, const float* boxes, const uint8_t* valid, const double* loc, const double* rot, const double* grot,
                                int num_try, const int32_t* box_off_h, int nb, int32_t* sel, double* sel_loc, double* sel_rot, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (nb < 1) return pp_fail(ctx, PP_E_ARG, "pp_augment_noise: nb must be >= 1");
    if (num_try < 1 || num_try > PP_AUG_MAX_TRIES) return pp_fail(ctx, PP_E_ARG, "pp_augment_noise: num_try must be 1 .. PP_AUG_MAX_TRIES");
    if (int rc = check_off(ctx, box_off_h, nb, PP_ASSIGN_MAX_GT, MAXB, "pp_augment_noise: null box_off_h")) return rc;
    const int G = box_off_h[nb];
    if (G == 0) return 0;
    if (!boxes || !valid || !loc || !rot || !grot || !sel || !sel_loc || !sel_rot) return pp_fail(ctx, PP_E_ARG, "pp_augment_noise: null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    for (int f0 = 0; f0 < nb; f0 += AUG_GROUP) {
        const int g = nb - f0 < AUG_GROUP ? nb - f0 : AUG_GROUP;
        const aug_args a = make_args(box_off_h, nullptr, f0, g, num_try, nullptr);
        hipLaunchKernelGGL(k_noise, dim3(g), dim3(NOISE_THREADS), 0, stream, a, boxes, valid, loc, rot, grot, sel, sel_loc, sel_rot);
    }
    PP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pp_augment_boxes(pp_ctx* ctx, const float* boxes, const int32_t* cls, const uint8_t* valid, const double* sel_loc,
                                const double* sel_rot, const double* prm, const float* range_h, const int32_t* box_off_h, int nb, float* out,
                                int32_t* out_cls, uint8_t* keep, int32_t* kept, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (nb < 1) return pp_fail(ctx, PP_E_ARG, "pp_augment_boxes: nb must be >= 1");
    if (int rc = check_off(ctx, box_off_h, nb, PP_ASSIGN_MAX_GT, MAXB, "pp_augment_boxes: null box_off_h")) return rc;
    if (!prm || !range_h || !kept) return pp_fail(ctx, PP_E_ARG, "pp_augment_boxes: null pointer");
    if (box_off_h[nb] > 0 && (!boxes || !cls || !valid || !sel_loc || !sel_rot || !out || !out_cls || !keep))
        return pp_fail(ctx, PP_E_ARG, "pp_augment_boxes: null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    for (int f0 = 0; f0 < nb; f0 += AUG_GROUP) {
        const int g = nb - f0 < AUG_GROUP ? nb - f0 : AUG_GROUP;
        const aug_args a = make_args(box_off_h, nullptr, f0, g, 0, range_h);
        hipLaunchKernelGGL(k_boxes, dim3(g), dim3(BOX_THREADS), 0, stream, a, boxes, cls, valid, sel_loc, sel_rot, prm, out, out_cls, keep, kept);
    }
    PP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pp_augment_points(pp_ctx* ctx, const float* pts, const int32_t* perm, const int32_t* pt_off_h, const float* boxes,
                                 const uint8_t* valid, const double* sel_loc, const double* sel_rot, const double* prm,
                                 const int32_t* box_off_h, int nb, float* out, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (nb < 1) return pp_fail(ctx, PP_E_ARG, "pp_augment_points: nb must be >= 1");
    if (int rc = check_off(ctx, box_off_h, nb, PP_ASSIGN_MAX_GT, MAXB, "pp_augment_points: null box_off_h")) return rc;
    if (int rc = check_off(ctx, pt_off_h, nb, 0x7FFFFFFF, 0, "pp_augment_points: null pt_off_h")) return rc;
    if (!prm) return pp_fail(ctx, PP_E_ARG, "pp_augment_points: null pointer");
    if (pt_off_h[nb] > 0 && (!pts || !out)) return pp_fail(ctx, PP_E_ARG, "pp_augment_points: null pointer");
    if (box_off_h[nb] > 0 && (!boxes || !valid || !sel_loc || !sel_rot)) return pp_fail(ctx, PP_E_ARG, "pp_augment_points: null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    for (int f0 = 0; f0 < nb; f0 += AUG_GROUP) {
        const int g = nb - f0 < AUG_GROUP ? nb - f0 : AUG_GROUP;
        const aug_args a = make_args(box_off_h, pt_off_h, f0, g, 0, nullptr);
        int maxn = 0;
        for (int z = 0; z < g; ++z) maxn = a.poff[z + 1] - a.poff[z] > maxn ? a.poff[z + 1] - a.poff[z] : maxn;
        if (maxn == 0) continue;
        hipLaunchKernelGGL(k_points, dim3(pp_div_up(maxn, PTS_THREADS * PTS_PER_THREAD), g), dim3(PTS_THREADS), 0, stream, a,
                           (const float4*)pts, perm, boxes, valid, sel_loc, sel_rot, prm, (float4*)out);
    }
    PP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pp_augment_draw(pp_ctx* ctx, uint64_t seed, uint32_t epoch, const int64_t* sample_h, int steps, int num_try,
                               const int32_t* box_off_h, int nb, double* loc, double* rot, double* grot, double* prm, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (nb < 1) return pp_fail(ctx, PP_E_ARG, "pp_augment_draw: nb must be >= 1");
    if (num_try < 1 || num_try > PP_AUG_MAX_TRIES) return pp_fail(ctx, PP_E_ARG, "pp_augment_draw: num_try must be 1 .. PP_AUG_MAX_TRIES");
    if (epoch >= (1u << 24)) return pp_fail(ctx, PP_E_ARG, "pp_augment_draw: epoch must be < 2^24");
    if (steps < 0 || steps > 127) return pp_fail(ctx, PP_E_ARG, "pp_augment_draw: steps must be a combination of the step bits");
    if (int rc = check_off(ctx, box_off_h, nb, PP_ASSIGN_MAX_GT, MAXB, "pp_augment_draw: null box_off_h")) return rc;
    if (!sample_h || !prm) return pp_fail(ctx, PP_E_ARG, "pp_augment_draw: null pointer");
    if (box_off_h[nb] > 0 && (!loc || !rot || !grot)) return pp_fail(ctx, PP_E_ARG, "pp_augment_draw: null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    for (int f0 = 0; f0 < nb; f0 += AUG_GROUP) {
        const int g = nb - f0 < AUG_GROUP ? nb - f0 : AUG_GROUP;
        draw_args a;
        std::memset(&a, 0, sizeof(a));
        a.f0 = f0;
        a.T = num_try;
        a.steps = steps;
        a.k0 = (uint32_t)seed;
        a.k1 = (uint32_t)(seed >> 32);
        a.epoch = epoch;
        int maxe = 1;
        for (int z = 0; z <= g; ++z) a.boff[z] = box_off_h[f0 + z];
        for (int z = 0; z < g; ++z) {
            a.sample[z] = sample_h[f0 + z];
            const int ne = (a.boff[z + 1] - a.boff[z]) * num_try;
            maxe = ne > maxe ? ne : maxe;
        }
        hipLaunchKernelGGL(k_draw, dim3(pp_div_up(maxe, 256), g), dim3(256), 0, stream, a, loc, rot, grot, prm);
    }
    PP_HIP(hipGetLastError());
    return 0;
}
