// Device-side self checks reachable through the C ABI (evplp_selftest): facts the kernels rely on, verified on the part they
// run on rather than assumed.
#include "device_common.hpp"
#include "context.hpp"
#include "ev_math.h"

namespace evplp {

// which = 0: rcp_exact(x) against the IEEE division 1.0f / x on ALL 2^32 bit patterns.
//   out[0] patterns where the bits differ (NaN == NaN), out[1] of them zero / denormal x, out[2] infinite / NaN x, out[3] normal x,
//   out[4] / out[5] smallest / largest biased exponent among the differing normal x (255 / 0 if none).
__global__ __launch_bounds__(256) void selftest_rcp_kernel(unsigned long long *out) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = tid; i < (1ull << 32); i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t b = (uint32_t)i;
        const float x = __uint_as_float(b);
        const float ref = 1.0f / x, got = rcp_exact(x);
        v2f xx; xx.x = x; xx.y = -x;
        const v2f g2 = rcp_exact2(xx);                                   // the packed flavour must agree with the scalar one
        const bool same = (__float_as_uint(ref) == __float_as_uint(got) || (ref != ref && got != got)) &&
                          (__float_as_uint(g2.x) == __float_as_uint(got) || (g2.x != g2.x && got != got)) &&
                          (__float_as_uint(g2.y) == (__float_as_uint(got) ^ 0x80000000u) || (g2.y != g2.y && got != got));
        if (!same) {
            const uint32_t ex = (b >> 23) & 0xffu;
            atomicAdd(&out[0], 1ull);
            if (ex == 0u) atomicAdd(&out[1], 1ull);
            else if (ex == 255u) atomicAdd(&out[2], 1ull);
            else { atomicAdd(&out[3], 1ull); atomicMin(&out[4], (unsigned long long)ex); atomicMax(&out[5], (unsigned long long)ex); }
        }
    }
}

// which = 1: d^e = exp2(e log2 d) on the hardware transcendentals (the Phong lobes of the VPL gather and of the splat) against the
// double-precision pow, for e = 1, 5, 20, 100, 1000, 10000 and 2^22 values of d in (1e-6, 1]: out[k] = the largest relative error over
// the d whose lobe is at least 1e-4 of its peak, in units of 1e-12.
__global__ __launch_bounds__(256) void selftest_pow_kernel(unsigned long long *out) {
    const float es[6] = { 1.0f, 5.0f, 20.0f, 100.0f, 1000.0f, 10000.0f };
    const uint32_t n = 1u << 22;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float d = 1.0f - (float)i / (float)n * 0.999999f;
        for (int k = 0; k < 6; k++) {
            const double want = pow((double)d, (double)es[k]);
            if (want < 1e-4) continue;
            const double got = (double)__builtin_amdgcn_exp2f(es[k] * __builtin_amdgcn_logf(d));
            const double rel = fabs(got - want) / want;
            atomicMax(&out[k], (unsigned long long)(rel * 1e12));
        }
    }
}

// which = 2: the hand-written triangle-pair test of the packet walks (device_common.hpp EV_PAIR_TEXT, through pair_hits_asm) against
// tri_pair_test, its C++ statement, on the same inputs: kPairTestPairs pairs x 64 directions, generated here from a fixed seed, in six
// classes (pair index mod 6):
//   0 random triangles and segments                      3 scales 2^-41 .. 2^-44: the denominator n . d crosses into the denormals
//   1 small-integer coordinates, bounds 1/8 and 1/2      4 as 0 with an all-zero B half (the padding of a one- or three-triangle leaf)
//   2 as 1 (a quarter of the lanes: den = 0, below)      5 coordinates scaled by 1e-15, 1e-12, 1e12, 1e15
// In every class lanes 0-31 aim at triangle A and lanes 32-63 at triangle B: at the point p0 + b (p1 - p0) + c (p2 - p0) with (b, c) from
// a 4 x 4 grid of eighths that holds the vertices (0, 0) (1, 0) (0, 1), edge points (b = 0, c = 0, b + c = 1) and interior and exterior
// points, reached at t = 1/4, or 1/8, or 1/2 (d = (P - o) / t: exact for the integer classes, where t then lands exactly on the
// bounds); odd lanes of class 2 run along the plane instead (d = i e0 + j e1, den = 0 exactly).
// out[0] lanes x triangles whose hit bit differs (both register layouts, VT = 52 and 116), out[1] cases, out[2] hits (tri_pair_test's),
// out[3] / [4] / [5] = hits of classes 0 | 1 << 32, 2 | 3 << 32, 4 | 5 << 32.
constexpr uint32_t kPairTestPairs = 4096u;
struct PairTestRec { float tri[24]; float o[3]; float tmin, tmax; uint32_t cls; uint32_t pad[2]; };      // 128 bytes: two s_load_dwordx16
static_assert(sizeof(PairTestRec) == 128, "PairTestRec");
EV_DEV float pt_uniform(uint64_t &st) { st = splitmix64(st); return (float)(st >> 40) * (1.0f / 16777216.0f); }
EV_DEV float pt_int(uint64_t &st, int lim) { st = splitmix64(st); return (float)((int)((st >> 33) % (uint64_t)(2 * lim + 1)) - lim); }
__global__ __launch_bounds__(64) void selftest_pair_gen_kernel(PairTestRec *recs) {
    const uint32_t pair = blockIdx.x * 64u + threadIdx.x;
    if (pair >= kPairTestPairs) return;
    PairTestRec r = {};
    const uint32_t cls = pair % 6u;
    uint64_t st = 0x5eedull * 0x10001ull + pair;
    const bool ints = cls == 1u || cls == 2u;
    float scale = 1.0f;
    if (cls == 3u) scale = __builtin_ldexpf(1.0f, -41 - (int)((pair / 6u) & 3u));
    if (cls == 5u) { const float sc[4] = { 1e-15f, 1e-12f, 1e12f, 1e15f }; scale = sc[(pair / 6u) & 3u]; }
    for (int h = 0; h < 2; h++) {
        float v[9];
        for (int k = 0; k < 9; k++) v[k] = (ints ? pt_int(st, 4) : 2.0f * pt_uniform(st) - 1.0f) * scale;
        if (h == 1 && cls == 4u) continue;          // the B half stays all zeros
        // (evplp_build_accel's precompute_tri: e0 = p1 - p0, e1 = p0 - p2, n = cross(e1, e0))
        float e0[3], e1[3];
        for (int k = 0; k < 3; k++) { e0[k] = v[3 + k] - v[k]; e1[k] = v[k] - v[6 + k]; }
        const float n[3] = { e1[1] * e0[2] - e1[2] * e0[1], e1[2] * e0[0] - e1[0] * e0[2], e1[0] * e0[1] - e1[1] * e0[0] };
        for (int k = 0; k < 3; k++) { r.tri[2 * k + h] = v[k]; r.tri[6 + 2 * k + h] = e0[k]; r.tri[12 + 2 * k + h] = e1[k]; r.tri[18 + 2 * k + h] = n[k]; }
    }
    for (int k = 0; k < 3; k++) r.o[k] = (ints ? pt_int(st, 8) : 4.0f * pt_uniform(st) - 2.0f) * scale;
    r.tmin = ints ? 0.125f : 0.0001f; r.tmax = ints ? 0.5f : 1.0f - 0.0001f;
    r.cls = cls;
    recs[pair] = r;
}
template <int VT> EV_DEV void selftest_pair_body(const PairTestRec *recs, unsigned long long *out) {
#pragma clang fp contract(off)
    const uint32_t pair = blockIdx.x, lane = threadIdx.x & 63u;
    v16i a, b;
    sload16x2(recs, pair * (uint32_t)sizeof(PairTestRec), a, b);
    PairOps P;
    P.p0x = pk(a[0], a[1]); P.p0y = pk(a[2], a[3]); P.p0z = pk(a[4], a[5]); P.e0x = pk(a[6], a[7]); P.e0y = pk(a[8], a[9]); P.e0z = pk(a[10], a[11]);
    P.e1x = pk(a[12], a[13]); P.e1y = pk(a[14], a[15]); P.e1z = pk(b[0], b[1]); P.nx = pk(b[2], b[3]); P.ny = pk(b[4], b[5]); P.nz = pk(b[6], b[7]);
    const V3 o = v3(f_of(b[8]), f_of(b[9]), f_of(b[10]));
    const float tmin = f_of(b[11]), tmax = f_of(b[12]);
    const uint32_t cls = (uint32_t)b[13];
    // this lane's direction
    const int h = (int)(lane >> 5);
    const uint32_t q = lane & 31u;
    const float p0[3] = { h ? P.p0x.y : P.p0x.x, h ? P.p0y.y : P.p0y.x, h ? P.p0z.y : P.p0z.x };
    const float e0[3] = { h ? P.e0x.y : P.e0x.x, h ? P.e0y.y : P.e0y.x, h ? P.e0z.y : P.e0z.x };
    const float e1[3] = { h ? P.e1x.y : P.e1x.x, h ? P.e1y.y : P.e1y.x, h ? P.e1z.y : P.e1z.x };
    float dd[3];
    if (cls == 2u && (q & 1u)) {
        const float i = (float)((int)(q >> 1) % 4 - 1), j = (float)((int)(q >> 3) + 1);
        for (int k = 0; k < 3; k++) dd[k] = i * e0[k] + j * e1[k];
    } else {
        const float bs[4] = { 0.0f, 0.5f, 1.0f, 0.25f }, cs[4] = { 0.0f, 0.5f, 0.25f, 1.0f };
        const float bb = bs[q & 3u], cc = cs[(q >> 2) & 3u];
        const float inv_t = (q >> 4) == 0u ? 4.0f : ((pair >> 3) & 1u ? 8.0f : 2.0f);
        // P = p0 + b (p1 - p0) + c (p2 - p0) = p0 + b e0 - c e1
        for (int k = 0; k < 3; k++) dd[k] = ((p0[k] + bb * e0[k] - cc * e1[k]) - (k == 0 ? o.x : k == 1 ? o.y : o.z)) * inv_t;
    }
    const V3 d = v3(dd[0], dd[1], dd[2]);
    unsigned long long ha, hb;
    pair_hits_asm<VT>(P, o, d, tmin, tmax, ha, hb);
    const Hit2 ref = tri_pair_test(P.p0x, P.p0y, P.p0z, P.e0x, P.e0y, P.e0z, P.e1x, P.e1y, P.e1z, P.nx, P.ny, P.nz, o, d, tmin, tmax);
    const unsigned long long ra = ballot64(ref.a), rb = ballot64(ref.b);
    if (lane == 0u) {
        const unsigned long long bad = (unsigned long long)(__builtin_popcountll(ha ^ ra) + __builtin_popcountll(hb ^ rb));
        const unsigned long long hits = (unsigned long long)(__builtin_popcountll(ra) + __builtin_popcountll(rb));
        if (bad) atomicAdd(&out[0], bad);
        atomicAdd(&out[1], 128ull);
        atomicAdd(&out[2], hits);
        atomicAdd(&out[3 + cls / 2u], hits << (32u * (cls & 1u)));
    }
}
// (the attribute takes a literal: one kernel per register layout, as the walks have -- v[50:63] and v[116:127])
__attribute__((amdgpu_num_vgpr(50))) __global__ __launch_bounds__(64) void selftest_pair52_kernel(const PairTestRec *recs, unsigned long long *out) { selftest_pair_body<52>(recs, out); }
__attribute__((amdgpu_num_vgpr(116))) __global__ __launch_bounds__(64) void selftest_pair116_kernel(const PairTestRec *recs, unsigned long long *out) { selftest_pair_body<116>(recs, out); }

// which = 3: the in-place visit of a synthetic node (device_common.hpp EV_SYN_VISIT_ASM_: the node read from LDS into the visit's own
// registers) against the scalar-operand visit EV_WALK_VISIT_ASM_ on the same node and rays: kSynTestNodes nodes x 64 rays that share their
// origin (as the lanes of a gather wave do), generated here from a fixed seed, in six classes (node index mod 6):
//   0 random boxes around random segments                          3 child 0 ends exactly at a segment end point: its face in the plane
//   1 the second entry absent, as the cut kernel writes an odd       of the shared origin, or of the end points (which then share their x):
//     count: reference kNoChild, centre 0, half-size -3e38           entry == exit after the clamp, not entered from that side
//   2 as 0, a quarter of the lanes dead (+inf origin terms)        4 child 0 with zero half-sizes (a point, or flat in x)
//                                                                  5 as 0, coordinates scaled by 1e-15, 1e-12, 1e12, 1e15
// Where a class shapes child 0, child 1 is a box of class 0.  Every visit starts from a stack of (node index mod 4) entries in a register
// whose 64 lanes all differ, so that a wrong push, pop or stack pointer shows.  Compared: both entered-lane masks, the next node
// reference, the stack pointer and the stack register (all 64 lanes: the pushed entry and everything a push must leave alone).
// out[0] differences (mask bits + references + stack pointers + stack lanes), out[1] cases (lanes x children), out[2] entered lanes x
// children (the reference visit's), out[3] / [4] / [5] = entered of classes 0 | 1 << 32, 2 | 3 << 32, 4 | 5 << 32.
constexpr uint32_t kSynTestNodes = 4096u;
struct SynTestRec { float node[12]; int32_t c0, c1; uint32_t pad0[2]; float o[3], q[3], spread; uint32_t cls, flat_x, sp0; uint32_t pad1[6]; };   // 128 bytes
static_assert(sizeof(SynTestRec) == 128, "SynTestRec");
__global__ __launch_bounds__(64) void selftest_syn_gen_kernel(SynTestRec *recs) {
    const uint32_t node = blockIdx.x * 64u + threadIdx.x;
    if (node >= kSynTestNodes) return;
    SynTestRec r = {};
    const uint32_t cls = node % 6u, odd = (node / 6u) & 1u;
    uint64_t st = 0xc07ull * 0x10001ull + node;
    float S = 1.0f;
    if (cls == 5u) { const float sc[4] = { 1e-15f, 1e-12f, 1e12f, 1e15f }; S = sc[(node / 6u) & 3u]; }
    float o[3], q[3];
    // (multiples of 1/64: the faces of class 3 are then exact sums)
    for (int k = 0; k < 3; k++) { o[k] = floorf((4.0f * pt_uniform(st) - 2.0f) * 64.0f) * (1.0f / 64.0f) * S; q[k] = floorf((4.0f * pt_uniform(st) - 2.0f) * 64.0f) * (1.0f / 64.0f) * S; }
    for (int e = 0; e < 2; e++) {
        // a box about a point of the segment origin -> target centre, off it by up to 0.2, half-sizes 0.1 .. 0.5; the targets of the 64
        // lanes spread over +-1 about the centre: a third to a half of the lanes pass through it
        const float along = 0.2f + 0.6f * pt_uniform(st);
        for (int k = 0; k < 3; k++) {
            r.node[2 * k + e] = o[k] + along * (q[k] - o[k]) + (pt_uniform(st) - 0.5f) * 0.4f * S;
            r.node[6 + 2 * k + e] = (0.1f + 0.4f * pt_uniform(st)) * S;
        }
    }
    r.c0 = (node & 1u) ? ~(int32_t)(node * 4u + 1u) : (int32_t)(node * 2u + 1u);       // (a leaf reference or a node index: the visit only passes them on)
    r.c1 = (int32_t)(node * 2u + 2u);
    if (cls == 1u) { r.c1 = kNoChild; for (int k = 0; k < 3; k++) { r.node[2 * k + 1] = 0.0f; r.node[6 + 2 * k + 1] = -3.0e38f; } }
    if (cls == 3u) {
        // x: [o.x - 1/2, o.x] (behind the origin of a lane that looks along +x) or [q.x, q.x + 1/2] (beyond its end point); y, z: wide
        const float *at = odd ? q : o;
        r.node[0] = odd ? q[0] + 0.25f : o[0] - 0.25f; r.node[6] = 0.25f;
        for (int k = 1; k < 3; k++) { r.node[2 * k] = at[k]; r.node[6 + 2 * k] = 4.0f; }
        r.flat_x = odd;
    }
    if (cls == 4u) { r.node[6] = 0.0f; if (!odd) { r.node[8] = 0.0f; r.node[10] = 0.0f; } }
    for (int k = 0; k < 3; k++) { r.o[k] = o[k]; r.q[k] = q[k]; }
    r.spread = 2.0f * S; r.cls = cls; r.sp0 = node & 3u;
    recs[node] = r;
}
// The node visit of the walk (device_common.hpp EV_VISIT_TEXT, the very text EV_WALK_LOOP_ASM executes) as a statement of its own, with
// operands in place of the walk's fixed scalar registers.  NC: the constraint of the node's six box operands ("s": register pairs of a
// node fetched with a scalar load).  TAIL: text behind the visit (the first mask is copied out of vcc there).
// (the text names no %[lane]: the operand only keeps the lane id in a register across the statement)
#define EV_WALK_VISIT_ASM_(NC, TAIL, T0, T1, T2, T3, T4, T5, T0L, T0H, T1L, T1H, T2L, T2H, T3L, T3H, T4L, T4H, T5L, T5H)                         \
    asm volatile(                                                                                                                            \
        EV_VISIT_TEXT("%[cx]", "%[cy]", "%[cz]", "%[hx]", "%[hy]", "%[hz]", "%[c0]", "%[c1]", "%[m1]", "%[t64]", "%[p0]", "%[p1]",           \
                      T0, T1, T2, T3, T4, T5, T0L, T0H, T1L, T1H, T2L, T2H, T3L, T3H, T4L, T4H, T5L, T5H)                                    \
        TAIL                                                                                                                                 \
        : [cur] "+s"(cur), [sp] "+s"(sp), [vstack] "+v"(vstack), [m1] "=&s"(m1_), [t64] "=&s"(t64_), [p0] "=&s"(p0_), [p1] "=&s"(p1_)          \
        : [cx] NC(cx_), [cy] NC(cy_), [cz] NC(cz_), [hx] NC(hx_), [hy] NC(hy_), [hz] NC(hz_), [c0] "s"(c0_), [c1] "s"(c1_),              \
          [pa] "v"(pa_), [pb] "v"(pb_), [pc] "v"(pc_),                                     \
          [pd] "v"(pd_), [pe] "v"(pe_), [lane] "v"(lane_id)                                                                 \
        : "vcc", "scc", "m0", T0L, T0H, T1L, T1H, T2L, T2H, T3L, T3H, T4L, T4H, T5L, T5H)
__attribute__((amdgpu_num_vgpr(50))) __global__ __launch_bounds__(64) void selftest_syn_kernel(const SynTestRec *recs, unsigned long long *out) {
    __shared__ float4 s_node[4];
    const uint32_t node = blockIdx.x, lane = threadIdx.x & 63u;
    if (lane < 16u) reinterpret_cast<int32_t *>(s_node)[lane] = reinterpret_cast<const int32_t *>(recs)[node * 32u + lane];
    __syncthreads();
    v16i N, b;
    sload16x2(recs, node * (uint32_t)sizeof(SynTestRec), N, b);
    const V3 o = v3(f_of(b[0]), f_of(b[1]), f_of(b[2])), q = v3(f_of(b[3]), f_of(b[4]), f_of(b[5]));
    const float spread = f_of(b[6]);
    const uint32_t cls = (uint32_t)b[7], flat_x = (uint32_t)b[8];
    const int sp0 = b[9];
    // this lane's ray: from the shared origin to its own target about q
    uint64_t st = 0xa11ull * 0x10001ull + (uint64_t)node * 64u + lane;
    const float ux = pt_uniform(st) - 0.5f, uy = pt_uniform(st) - 0.5f, uz = pt_uniform(st) - 0.5f;
    const V3 d = v3((q.x + (flat_x ? 0.0f : spread * ux)) - o.x, (q.y + spread * uy) - o.y, (q.z + spread * uz) - o.z);
    st = splitmix64(st);
    const bool alive_lane = !(cls == 2u && (st >> 62) == 0ull);
    // the ray constants as occluded_wave sets them up
    const float tmin = 0.0001f, tmax = 1.0f - 0.0001f;
    const V3 inv0 = v3(safe_rcp(d.x), safe_rcp(d.y), safe_rcp(d.z));
    const float ku = 1.0f / (tmax - tmin);
    const V3 inv = inv0 * ku;
    const float dead = __builtin_inff();
    v2f pa_, pb_, pc_, pd_, pe_;
    pa_.x = inv.x; pa_.y = inv.y; pb_.x = inv.z; pb_.y = fabsf(inv.x); pc_.x = fabsf(inv.y); pc_.y = fabsf(inv.z);
    pd_.x = alive_lane ? (-(o.x * inv0.x) - tmin) * ku : dead; pd_.y = alive_lane ? (-(o.y * inv0.y) - tmin) * ku : dead;
    pe_.x = alive_lane ? (-(o.z * inv0.z) - tmin) * ku : dead; pe_.y = pe_.x;
    const int lane_id = (int)lane;
    const int vstack0 = 0x01000000 + (int)(node * 64u + lane);
    // the reference: the node in scalar registers (the first mask is copied out of vcc into the dead temporary pair)
    unsigned long long ref_m0, ref_m1; int32_t ref_cur; int ref_sp, ref_stack;
    {
        const v2f cx_ = pk(N[0], N[1]), cy_ = pk(N[2], N[3]), cz_ = pk(N[4], N[5]), hx_ = pk(N[6], N[7]), hy_ = pk(N[8], N[9]), hz_ = pk(N[10], N[11]);
        const int32_t c0_ = N[12], c1_ = N[13];
        unsigned long long m1_, t64_; int32_t p0_, p1_;
        int32_t cur = 0; int sp = sp0, vstack = vstack0;
        EV_WITH(EV_WALK_VISIT_ASM_, "s", "s_mov_b64 %[t64], vcc\n", EV_TMP_52);
        ref_m0 = t64_; ref_m1 = m1_; ref_cur = cur; ref_sp = sp; ref_stack = vstack;
    }
    // the subject: the node from LDS, in place, with the dead lanes of class 2 outside EXEC as the walk runs it (the reference visit above
    // keeps EXEC full and relies on their +inf origin terms: the same masks either way)
    unsigned long long got_m0, got_m1; int32_t got_cur; int got_sp, got_stack;
    {
        const unsigned long long alive = ballot64(alive_lane);
        const uint32_t syn_addr_ = lds_offset(&s_node[0]);
        unsigned long long m1_, t64_; int32_t p0_, p1_, c0_, c1_;
        int32_t cur = 0; int sp = sp0, vstack = vstack0;
        EV_SYN_VISIT_ASM_("s_mov_b64 %[t64], vcc\n");
        got_m0 = t64_; got_m1 = m1_; got_cur = cur; got_sp = sp; got_stack = vstack;
    }
    const unsigned long long stack_bad = ballot64(got_stack != ref_stack);
    if (lane == 0u) {
        const unsigned long long bad = (unsigned long long)(__builtin_popcountll(got_m0 ^ ref_m0) + __builtin_popcountll(got_m1 ^ ref_m1) + __builtin_popcountll(stack_bad)) +
                                       (got_cur != ref_cur ? 1ull : 0ull) + (got_sp != ref_sp ? 1ull : 0ull);
        const unsigned long long entered = (unsigned long long)(__builtin_popcountll(ref_m0) + __builtin_popcountll(ref_m1));
        if (bad) atomicAdd(&out[0], bad);
        atomicAdd(&out[1], 128ull);
        atomicAdd(&out[2], entered);
        atomicAdd(&out[3 + cls / 2u], entered << (32u * (cls & 1u)));
    }
}

// which = 5: the whole hand-written walk (device_common.hpp occluded_wave<false>: EV_WALK_LOOP_ASM with EXEC = the live lanes) against the C++
// walk (occluded_wave_ref<false>, full EXEC and +inf origin terms) on the same packet, one after the other: kWalkTestPackets packets of 64
// rays with a shared origin through a tree generated here from a fixed seed -- a complete binary tree over kWalkTestLeaves leaves of 1 - 4
// small triangles, one leaf per cell of an 8 x 8 x 4 grid over [-1, 1]^3 in Morton order, 255 inner nodes.  The lanes that start alive, by
// class (packet index mod 8):
//   0 all 64        2 lanes 32-63 (0-31 dead)     4 only lane 63     6 a random quarter
//   1 all but 0     3 lanes 0-31 (32-63 dead)     5 only lane 0      7 none (both walks return at once)
// out[0] lanes whose answers differ + lanes missing from EXEC behind the walk (must be 0), out[1] cases (lanes), out[2] occluded lanes (the C++
// walk's), out[3] / [4] / [5] = those of classes 0 | 1 << 21 | 2 << 42, 3 | 4 << 21 | 5 << 42, 6 | 7 << 21.
constexpr uint32_t kWalkTestLeaves = 256u, kWalkTestPackets = 4096u;
EV_DEV uint32_t wt_leaf_count(uint32_t leaf) { return (uint32_t)(splitmix64(0x1eafull * 0x10001ull + leaf) >> 62) + 1u; }
__global__ __launch_bounds__(256) void selftest_walk_gen_kernel(float *nodes, float *leaves) {
    __shared__ float s_lo[2u * kWalkTestLeaves - 1u][3], s_hi[2u * kWalkTestLeaves - 1u][3];
    const uint32_t k = threadIdx.x;                     // leaf k = heap node kWalkTestLeaves - 1 + k
    {
        uint32_t cell[3] = { 0u, 0u, 0u };
        for (uint32_t bit = 0; bit < 8u; bit++) { const uint32_t ax = bit < 6u ? bit % 3u : bit - 6u; cell[ax] |= ((k >> bit) & 1u) << (bit < 6u ? bit / 3u : 2u); }      // (x, y: three bits, z: two)
        const float ctr[3] = { -1.0f + ((float)cell[0] + 0.5f) * 0.25f, -1.0f + ((float)cell[1] + 0.5f) * 0.25f, -1.0f + ((float)cell[2] + 0.5f) * 0.5f };
        const uint32_t cnt = wt_leaf_count(k);
        uint64_t st = 0x7417ull * 0x10001ull + k;
        float blk[48];
        for (int q = 0; q < 48; q++) blk[q] = 0.0f;       // an empty slot is all zeros: never a hit
        float lo[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, hi[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
        for (uint32_t j = 0; j < cnt; j++) {
            float v[9];
            for (int q = 0; q < 3; q++) v[q] = ctr[q] + (pt_uniform(st) - 0.5f) * 0.2f;
            for (int q = 3; q < 9; q++) v[q] = v[q % 3] + (pt_uniform(st) - 0.5f) * 0.4f;
            // (evplp_build_accel's precompute_tri: e0 = p1 - p0, e1 = p0 - p2, n = cross(e1, e0))
            float e0[3], e1[3];
            for (int q = 0; q < 3; q++) { e0[q] = v[3 + q] - v[q]; e1[q] = v[q] - v[6 + q]; }
            const float n[3] = { e1[1] * e0[2] - e1[2] * e0[1], e1[2] * e0[0] - e1[0] * e0[2], e1[0] * e0[1] - e1[1] * e0[0] };
            float *pr = blk + 24u * (j >> 1); const uint32_t h = j & 1u;
            for (int q = 0; q < 3; q++) { pr[2 * q + h] = v[q]; pr[6 + 2 * q + h] = e0[q]; pr[12 + 2 * q + h] = e1[q]; pr[18 + 2 * q + h] = n[q]; }
            for (int q = 0; q < 9; q++) { lo[q % 3] = fminf(lo[q % 3], v[q]); hi[q % 3] = fmaxf(hi[q % 3], v[q]); }
        }
        for (int q = 0; q < 48; q++) leaves[k * 48u + q] = blk[q];
        for (int q = 0; q < 3; q++) { s_lo[kWalkTestLeaves - 1u + k][q] = lo[q]; s_hi[kWalkTestLeaves - 1u + k][q] = hi[q]; }
    }
    for (uint32_t w = kWalkTestLeaves / 2u; w >= 1u; w >>= 1) {      // the levels bottom-up: w nodes, heap indices w - 1 .. 2 w - 2
        __syncthreads();
        if (k < w) {
            const uint32_t i = w - 1u + k;
            for (int q = 0; q < 3; q++) { s_lo[i][q] = fminf(s_lo[2u * i + 1u][q], s_lo[2u * i + 2u][q]); s_hi[i][q] = fmaxf(s_hi[2u * i + 1u][q], s_hi[2u * i + 2u][q]); }
        }
    }
    __syncthreads();
    if (k < kWalkTestLeaves - 1u) {
        // BvhNode: centres x x y y z z, half-sizes x x y y z z (child 0, child 1 next to each other), the two references, two padding words
        float *nd = nodes + k * 16u;
        for (uint32_t e = 0; e < 2u; e++) {
            const uint32_t ch = 2u * k + 1u + e;
            for (int q = 0; q < 3; q++) {
                nd[2 * q + e] = 0.5f * (s_lo[ch][q] + s_hi[ch][q]);
                nd[6 + 2 * q + e] = 0.5f * (s_hi[ch][q] - s_lo[ch][q]) * 1.00001f + 1.0e-6f;
            }
            const int32_t ref = ch < kWalkTestLeaves - 1u ? (int32_t)ch : ~(int32_t)(((ch - (kWalkTestLeaves - 1u)) << 2) | (wt_leaf_count(ch - (kWalkTestLeaves - 1u)) - 1u));
            nd[12 + e] = __int_as_float(ref);
        }
        nd[14] = 0.0f; nd[15] = 0.0f;
    }
}
__attribute__((amdgpu_num_vgpr(50))) __global__ __launch_bounds__(64) void selftest_walk_kernel(const float *nodes, const float *leaves, unsigned long long *out) {
    const uint32_t packet = blockIdx.x, lane = threadIdx.x & 63u, cls = packet & 7u;
    const char *node_base = reinterpret_cast<const char *>(nodes), *leaf_base = reinterpret_cast<const char *>(leaves);
    // the packet: a shared origin in or around the grid, every lane's end point about a common target inside it
    uint64_t st = 0x9ac7ull * 0x10001ull + packet;
    const V3 o = v3(3.0f * pt_uniform(st) - 1.5f, 3.0f * pt_uniform(st) - 1.5f, 3.0f * pt_uniform(st) - 1.5f);
    const V3 q = v3(2.0f * pt_uniform(st) - 1.0f, 2.0f * pt_uniform(st) - 1.0f, 2.0f * pt_uniform(st) - 1.0f);
    uint64_t sl = 0xa11ull * 0x10001ull + (uint64_t)packet * 64u + lane;
    const float ux = pt_uniform(sl) - 0.5f, uy = pt_uniform(sl) - 0.5f, uz = pt_uniform(sl) - 0.5f;
    const V3 d = v3((q.x + 0.8f * ux) - o.x, (q.y + 0.8f * uy) - o.y, (q.z + 0.8f * uz) - o.z);
    sl = splitmix64(sl);
    const bool alive_lane = cls == 0u ? true : cls == 1u ? lane != 0u : cls == 2u ? lane >= 32u : cls == 3u ? lane < 32u : cls == 4u ? lane == 63u :
                            cls == 5u ? lane == 0u : cls == 6u ? (sl >> 62) == 0ull : false;
    const float tmin = 0.0001f, tmax = 1.0f - 0.0001f;
    const bool got = occluded_wave<false>(node_base, leaf_base, o, d, tmin, tmax, alive_lane, nullptr, 0u);
    const unsigned long long exec_after = ballot64(true);               // every statement of the walk hands EXEC back full
    const bool ref = occluded_wave_ref<false>(node_base, leaf_base, o, d, tmin, tmax, alive_lane, nullptr, nullptr, 0u);
    const unsigned long long diff = ballot64(got != ref), occ = ballot64(ref);
    if (lane == 0u) {
        const unsigned long long bad = (unsigned long long)(__builtin_popcountll(diff) + __builtin_popcountll(~exec_after));
        const unsigned long long n_occ = (unsigned long long)__builtin_popcountll(occ);
        if (bad) atomicAdd(&out[0], bad);
        atomicAdd(&out[1], 64ull);
        atomicAdd(&out[2], n_occ);
        atomicAdd(&out[3 + cls / 3u], n_occ << (21u * (cls % 3u)));
    }
}

// which = 4: the hardware primitives of the VSL estimators (kernels_gather.hip, namespace vslm) against double precision; maxima in
// units of 1e-12:
//   out[0] / out[1]  |v_sin_f32(u) - sin(2 pi u)| / |v_cos_f32(u) - cos(2 pi u)| over all 2^24 uniforms u = (k + 1) 2^-24 (the
//                    azimuth of every sampled direction: square_to_solid_angle, lambert_local, phong_local)
//   out[2]           |exp2(log2(u) rcp(e + 1)) - u^(1 / (e + 1))| (phong_local's cos_t) for e = 0, 0.5, 1, 20, 200, 1000, 10000 over the
//                    2^22 uniforms u = (k + 1) 2^-22
//   out[3] / [4] / [5]  relative error of v_rcp_f32 / v_rsq_f32 / v_sqrt_f32 over 2^22 arguments spread evenly in the exponent over
//                    [2^-20, 2^20]
__global__ __launch_bounds__(256) void selftest_vsl_primitives_kernel(unsigned long long *out) {
    const float es[7] = { 0.0f, 0.5f, 1.0f, 20.0f, 200.0f, 1000.0f, 10000.0f };
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    double m[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (uint32_t k = tid; k < (1u << 24); k += stride) {
        const float u = (float)(k + 1u) * (1.0f / 16777216.0f);
        m[0] = fmax(m[0], fabs((double)__builtin_amdgcn_sinf(u) - sinpi(2.0 * (double)u)));
        m[1] = fmax(m[1], fabs((double)__builtin_amdgcn_cosf(u) - cospi(2.0 * (double)u)));
    }
    const uint32_t n = 1u << 22;
    for (uint32_t k = tid; k < n; k += stride) {
        const float u = (float)(k + 1u) * (1.0f / 4194304.0f);
        for (int j = 0; j < 7; j++) {
            float e1 = es[j] + 1.0f;
            asm volatile("" : "+v"(e1));               // (a run-time value, as in the kernels: the reciprocal of a constant would be folded, correctly rounded)
            const float got = __builtin_amdgcn_exp2f(__builtin_amdgcn_rcpf(e1) * __builtin_amdgcn_logf(u));
            m[2] = fmax(m[2], fabs((double)got - pow((double)u, 1.0 / ((double)es[j] + 1.0))));
        }
        const float x = (float)exp2(-20.0 + 40.0 * (double)k / (double)(n - 1u));
        m[3] = fmax(m[3], fabs((double)__builtin_amdgcn_rcpf(x) * (double)x - 1.0));
        m[4] = fmax(m[4], fabs((double)__builtin_amdgcn_rsqf(x) * sqrt((double)x) - 1.0));
        m[5] = fmax(m[5], fabs((double)__builtin_amdgcn_sqrtf(x) / sqrt((double)x) - 1.0));
    }
    for (int j = 0; j < 6; j++) atomicMax(&out[j], (unsigned long long)(m[j] * 1e12));
}

// evplp_debug_ev_math: ev_math.h's functions AS THE DEVICE COMPUTES THEM, on the caller's inputs.  The light-tracing records are compared with
// the oracle's byte for byte, and the oracle #includes the same header: that comparison vouches for the walk and the draw order, not for
// these functions -- unless the header really gives the same bits on both machines, which is what tests/test_gpu_parity.py checks with this
// entry point (device results against the oracle's gcc build of the header, dense grids over the callers' input ranges).
__global__ __launch_bounds__(256) void ev_math_kernel(int which, const float *x, const float *y, uint32_t n, float *o0, float *o1) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (which == 0) { float s, c; evm_sincosf(x[i], &s, &c); o0[i] = s; o1[i] = c; }
    else o0[i] = evm_powf(x[i], y[i]);
}

} // namespace evplp

extern "C" int evplp_debug_ev_math(evplp_context *c, int32_t which, const float *x, const float *y, int32_t n, float *out0, float *out1) {
    if (!c || !x || !out0 || n <= 0 || which < 0 || which > 1 || (which == 0 && !out1) || (which == 1 && !y)) { if (c) c->set_error("evplp_debug_ev_math: bad arguments"); return EVPLP_ERR_INVALID; }
    if (hipSetDevice(c->cfg.device) != hipSuccess) return EVPLP_ERR_HIP;
    float *d = nullptr;
    const size_t bytes = sizeof(float) * (size_t)n;
    if (hipMalloc((void **)&d, 4 * bytes) != hipSuccess) { (void)hipGetLastError(); c->set_error("evplp_debug_ev_math: out of memory"); return EVPLP_ERR_OOM; }
    float *dx = d, *dy = d + n, *d0 = d + 2 * (size_t)n, *d1 = d + 3 * (size_t)n;
    hipError_t e = hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && which == 1) e = hipMemcpy(dy, y, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(evplp::ev_math_kernel, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, c->stream, which, dx, dy, (uint32_t)n, d0, d1);
        e = hipStreamSynchronize(c->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(out0, d0, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess && which == 0) e = hipMemcpy(out1, d1, bytes, hipMemcpyDeviceToHost);
    hipFree(d);
    if (e != hipSuccess) { c->set_error("evplp_debug_ev_math: %s", hipGetErrorString(e)); return EVPLP_ERR_HIP; }
    return EVPLP_OK;
}

extern "C" int evplp_selftest(evplp_context *c, int32_t which, uint64_t *out, int32_t capacity) {
    if (!c || !out || capacity < 6 || which < 0 || which > 5) { if (c) c->set_error("evplp_selftest: bad arguments"); return EVPLP_ERR_INVALID; }
    if (hipSetDevice(c->cfg.device) != hipSuccess) return EVPLP_ERR_HIP;
    unsigned long long *d = nullptr;
    if (hipMalloc((void **)&d, 8 * sizeof(unsigned long long)) != hipSuccess) return EVPLP_ERR_OOM;
    const unsigned long long init[8] = { 0, 0, 0, 0, which == 0 ? 255ull : 0ull, 0, 0, 0 };
    hipError_t e = hipMemcpy(d, init, sizeof(init), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        if (which == 0) hipLaunchKernelGGL(evplp::selftest_rcp_kernel, dim3(4096), dim3(256), 0, c->stream, d);
        else if (which == 1) hipLaunchKernelGGL(evplp::selftest_pow_kernel, dim3(4096), dim3(256), 0, c->stream, d);
        else if (which == 4) hipLaunchKernelGGL(evplp::selftest_vsl_primitives_kernel, dim3(4096), dim3(256), 0, c->stream, d);
        else if (which == 3) {
            evplp::SynTestRec *recs = nullptr;
            e = hipMalloc((void **)&recs, sizeof(evplp::SynTestRec) * evplp::kSynTestNodes);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(evplp::selftest_syn_gen_kernel, dim3(evplp::kSynTestNodes / 64u), dim3(64), 0, c->stream, recs);
                hipLaunchKernelGGL(evplp::selftest_syn_kernel, dim3(evplp::kSynTestNodes), dim3(64), 0, c->stream, recs, d);
                e = hipStreamSynchronize(c->stream);
                hipFree(recs);
            }
        } else if (which == 5) {
            float *tree = nullptr;      // 256 node slots of 64 bytes (255 used), then the leaf blocks of 192 bytes
            e = hipMalloc((void **)&tree, 64u * evplp::kWalkTestLeaves + 192u * evplp::kWalkTestLeaves);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(evplp::selftest_walk_gen_kernel, dim3(1), dim3(evplp::kWalkTestLeaves), 0, c->stream, tree, tree + 16u * evplp::kWalkTestLeaves);
                hipLaunchKernelGGL(evplp::selftest_walk_kernel, dim3(evplp::kWalkTestPackets), dim3(64), 0, c->stream, tree, tree + 16u * evplp::kWalkTestLeaves, d);
                e = hipStreamSynchronize(c->stream);
                hipFree(tree);
            }
        } else {
            evplp::PairTestRec *recs = nullptr;
            e = hipMalloc((void **)&recs, sizeof(evplp::PairTestRec) * evplp::kPairTestPairs);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(evplp::selftest_pair_gen_kernel, dim3(evplp::kPairTestPairs / 64u), dim3(64), 0, c->stream, recs);
                hipLaunchKernelGGL(evplp::selftest_pair52_kernel, dim3(evplp::kPairTestPairs), dim3(64), 0, c->stream, recs, d);
                hipLaunchKernelGGL(evplp::selftest_pair116_kernel, dim3(evplp::kPairTestPairs), dim3(64), 0, c->stream, recs, d);
                e = hipStreamSynchronize(c->stream);
                hipFree(recs);
            }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    unsigned long long h[8] = {};
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    hipFree(d);
    if (e != hipSuccess) { c->set_error("evplp_selftest: %s", hipGetErrorString(e)); return EVPLP_ERR_HIP; }
    for (int k = 0; k < 6; k++) out[k] = h[k];
    return 6;
}
