// Micro-benchmark (developer tool): issue rate of the vector instructions the packet walk is made of, on gfx950, at 1 / 2 / 4 / 8
// waves per SIMD.  Every body is inline asm on eight independent registers (no dependence between consecutive instructions), so
// the compiler can neither fuse, pack nor drop anything.  Reported per line: nanoseconds per wave-instruction per SIMD from the event
// time of the launch (what a kernel pays), the clock the chip held inside the loop (s_memtime ticks / s_memrealtime ticks x 100 MHz,
// median over workgroups: the chip lowers its clock under load, by instruction mix) and their product, cycles per wave-instruction.
//   hipcc --offload-arch=gfx950 -O3 -Ievplp_amd/csrc -o tools/ub/valu tools/ub/valu.hip && tools/ub/valu > profiles/ub_valu_r04.txt
//   tools/ub/valu lanemoves > profiles/ub_valu_lanemoves.txt      (only v_readfirstlane_b32 / v_readlane_b32, with v_pk_fma_f32 beside them)
//   tools/ub/valu exec > profiles/ub_valu_exec.txt                (the walk's node visit and pair test under five EXEC / data arms, below)
#include <hip/hip_runtime.h>
#include "device_common.hpp"      // EV_VISIT_TEXT, EV_PAIR_TEXT, EV_TMP_52: the walk's own statements, for the EXEC modes
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>
using evplp::v2f;

enum { FMA, PK_FMA, PK_FMA_OPSEL, PK_MUL, MAX3, MAX3_CLAMP, CMP_VCC, CMP_SGPR, EXP, LOG, RCP, MOV, WRITELANE, MIX_VISIT, MUL_LO_U32, MAD_U64_U32, MUL_F32, SQRT, SIN, ALIGNBIT, READFIRSTLANE, READLANE, NMODES };
static const char *kNames[NMODES] = { "v_fma_f32", "v_pk_fma_f32", "v_pk_fma_f32 op_sel", "v_pk_mul_f32", "v_max3_f32", "v_max3_f32 clamp", "v_cmp_lt_f32 vcc",
                                      "v_cmp_lt_f32 s[..]", "v_exp_f32", "v_log_f32", "v_rcp_f32", "v_mov_b32", "v_writelane_b32", "node visit (9 pk_fma + 4 max3/min3 + 2 cmp)",
                                      "v_mul_lo_u32", "v_mad_u64_u32", "v_mul_f32", "v_sqrt_f32", "v_sin_f32", "v_alignbit_b32", "v_readfirstlane_b32", "v_readlane_b32 (constant lane)" };
static const int kPerIter[NMODES] = { 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 60, 64, 64, 64, 64, 64, 64, 64, 64 };

#define R8(OP) OP(0) OP(1) OP(2) OP(3) OP(4) OP(5) OP(6) OP(7)
template <int MODE> __global__ __launch_bounds__(256) void k(float *out, unsigned long long *cyc, float a, float b, int iters) {
    float x[8]; v2f p[8]; unsigned long long q[8];
    for (int j = 0; j < 8; j++) { x[j] = threadIdx.x + j; p[j].x = x[j]; p[j].y = x[j] + 0.5f; q[j] = threadIdx.x * 77u + j; }
    v2f pa = { a, a * 1.5f }, pb = { b, b * 0.5f };
    unsigned long long sg = 0;
    int sl[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };      // (lane-to-scalar moves: eight destinations of their own)
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (MODE == FMA) {
#define OP(j) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x[j]) : "v"(a), "v"(b));
                R8(OP)
#undef OP
            } else if (MODE == PK_FMA) {
#define OP(j) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(p[j]) : "v"(pa), "v"(pb));
                R8(OP)
#undef OP
            } else if (MODE == PK_FMA_OPSEL) {
#define OP(j) asm volatile("v_pk_fma_f32 %0, %0, %1, %2 op_sel:[0,1,0] op_sel_hi:[1,1,1] neg_lo:[0,1,0] neg_hi:[0,1,0]" : "+v"(p[j]) : "v"(pa), "v"(pb));
                R8(OP)
#undef OP
            } else if (MODE == PK_MUL) {
#define OP(j) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(p[j]) : "v"(pa));
                R8(OP)
#undef OP
            } else if (MODE == MAX3) {
#define OP(j) asm volatile("v_max3_f32 %0, %0, %1, %2" : "+v"(x[j]) : "v"(a), "v"(b));
                R8(OP)
#undef OP
            } else if (MODE == MAX3_CLAMP) {
#define OP(j) asm volatile("v_max3_f32 %0, %0, %1, %2 clamp" : "+v"(x[j]) : "v"(a), "v"(b));
                R8(OP)
#undef OP
            } else if (MODE == CMP_VCC) {
#define OP(j) asm volatile("v_cmp_lt_f32 vcc, %0, %1" : : "v"(x[j]), "v"(a) : "vcc");
                R8(OP)
#undef OP
            } else if (MODE == CMP_SGPR) {
#define OP(j) asm volatile("v_cmp_lt_f32 %0, %1, %2" : "=s"(sg) : "v"(x[j]), "v"(a));
                R8(OP)
#undef OP
            } else if (MODE == EXP) {
#define OP(j) asm volatile("v_exp_f32 %0, %0" : "+v"(x[j]));
                R8(OP)
#undef OP
            } else if (MODE == LOG) {
#define OP(j) asm volatile("v_log_f32 %0, %0" : "+v"(x[j]));
                R8(OP)
#undef OP
            } else if (MODE == RCP) {
#define OP(j) asm volatile("v_rcp_f32 %0, %0" : "+v"(x[j]));
                R8(OP)
#undef OP
            } else if (MODE == MOV) {
#define OP(j) asm volatile("v_mov_b32 %0, %1" : "+v"(x[j]) : "v"(a));
                R8(OP)
#undef OP
            } else if (MODE == MUL_LO_U32) {
#define OP(j) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(x[j]) : "v"(a));
                R8(OP)
#undef OP
            } else if (MODE == MAD_U64_U32) {      // the 64-bit multiply-add an LCG step is made of (plus two v_mul_lo_u32 for the high word)
#define OP(j) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(q[j]) : "v"(a), "v"(b) : "vcc");
                R8(OP)
#undef OP
            } else if (MODE == MUL_F32) {
#define OP(j) asm volatile("v_mul_f32 %0, %0, %1" : "+v"(x[j]) : "v"(a));
                R8(OP)
#undef OP
            } else if (MODE == SQRT) {
#define OP(j) asm volatile("v_sqrt_f32 %0, %0" : "+v"(x[j]));
                R8(OP)
#undef OP
            } else if (MODE == SIN) {
#define OP(j) asm volatile("v_sin_f32 %0, %0" : "+v"(x[j]));
                R8(OP)
#undef OP
            } else if (MODE == ALIGNBIT) {
#define OP(j) asm volatile("v_alignbit_b32 %0, %0, %0, %1" : "+v"(x[j]) : "v"(a));
                R8(OP)
#undef OP
            } else if (MODE == READFIRSTLANE) {      // (one statement for the eight: between statements the compiler pads every lane-to-scalar move with an s_nop)
                asm volatile("v_readfirstlane_b32 %0, %8\n\tv_readfirstlane_b32 %1, %9\n\tv_readfirstlane_b32 %2, %10\n\tv_readfirstlane_b32 %3, %11\n\tv_readfirstlane_b32 %4, %12\n\tv_readfirstlane_b32 %5, %13\n\tv_readfirstlane_b32 %6, %14\n\tv_readfirstlane_b32 %7, %15" : "=s"(sl[0]), "=s"(sl[1]), "=s"(sl[2]), "=s"(sl[3]), "=s"(sl[4]), "=s"(sl[5]), "=s"(sl[6]), "=s"(sl[7]) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]));
            } else if (MODE == READLANE) {
                asm volatile("v_readlane_b32 %0, %8, 5\n\tv_readlane_b32 %1, %9, 5\n\tv_readlane_b32 %2, %10, 5\n\tv_readlane_b32 %3, %11, 5\n\tv_readlane_b32 %4, %12, 5\n\tv_readlane_b32 %5, %13, 5\n\tv_readlane_b32 %6, %14, 5\n\tv_readlane_b32 %7, %15, 5" : "=s"(sl[0]), "=s"(sl[1]), "=s"(sl[2]), "=s"(sl[3]), "=s"(sl[4]), "=s"(sl[5]), "=s"(sl[6]), "=s"(sl[7]) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]));
            } else if (MODE == WRITELANE) {
                int sp = (i + u) & 63, val = i;
#define OP(j) asm volatile("s_mov_b32 m0, %1\n\tv_writelane_b32 %0, %2, m0" : "+v"(x[j]) : "s"(sp), "s"(val) : "m0");
                R8(OP)
#undef OP
            }
        }
        if (MODE == MIX_VISIT) {
            // the vector instructions of one node visit of the packet walk, in its order, on registers of their own (4 copies per iteration)
#pragma unroll
            for (int u = 0; u < 4; u++) {
                asm volatile(
                    "v_pk_fma_f32 %0, %10, %11, %12 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
                    "v_pk_fma_f32 %1, %10, %11, %12 op_sel:[0,1,1] op_sel_hi:[1,1,1]\n\t"
                    "v_pk_fma_f32 %2, %10, %12, %11 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
                    "v_pk_fma_f32 %3, %10, %12, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1] neg_lo:[0,1,0] neg_hi:[0,1,0]\n\t"
                    "v_pk_fma_f32 %4, %10, %11, %1 op_sel:[0,0,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0] neg_hi:[0,1,0]\n\t"
                    "v_pk_fma_f32 %5, %10, %11, %2 op_sel:[0,1,0] op_sel_hi:[1,1,1] neg_lo:[0,1,0] neg_hi:[0,1,0]\n\t"
                    "v_pk_fma_f32 %0, %10, %12, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
                    "v_pk_fma_f32 %1, %10, %11, %1 op_sel:[0,0,0] op_sel_hi:[1,0,1]\n\t"
                    "v_pk_fma_f32 %2, %10, %11, %2 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
                    "v_max3_f32 %7, %7, %8, %9 clamp\n\t"
                    "v_min3_f32 %8, %8, %9, %7 clamp\n\t"
                    "v_max3_f32 %9, %9, %7, %8 clamp\n\t"
                    "v_min3_f32 %7, %7, %8, %9 clamp\n\t"
                    "v_cmp_lt_f32 vcc, %7, %8\n\t"
                    "v_cmp_lt_f32 %6, %9, %7\n\t"
                    : "+v"(p[0]), "+v"(p[1]), "+v"(p[2]), "+v"(p[3]), "+v"(p[4]), "+v"(p[5]), "+s"(sg), "+v"(x[0]), "+v"(x[1]), "+v"(x[2])
                    : "s"(pa), "v"(pb), "v"(p[6])
                    : "vcc");
            }
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
    float s = (float)(sg & 1);
    for (int j = 0; j < 8; j++) s += x[j] + p[j].x + p[j].y + (float)(q[j] & 0xffull) + (float)(sl[j] & 1);
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if (threadIdx.x == 0) { cyc[2 * blockIdx.x] = t1 - t0; cyc[2 * blockIdx.x + 1] = r1 - r0; }
}

template <int MODE> void run(int waves_per_simd, FILE *f) {
    const int grid = 256 * waves_per_simd, iters = 4000;
    float *out; unsigned long long *cyc;
    hipMalloc(&out, (size_t)grid * 256 * 4); hipMalloc(&cyc, (size_t)grid * 16);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    k<MODE><<<grid, 256>>>(out, cyc, 1.0001f, 0.5f, 10);
    hipEventRecord(e0); k<MODE><<<grid, 256>>>(out, cyc, 1.0001f, 0.5f, iters); hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    std::vector<unsigned long long> h((size_t)grid * 2); hipMemcpy(h.data(), cyc, (size_t)grid * 16, hipMemcpyDeviceToHost);
    std::vector<double> ghz((size_t)grid);
    for (int b = 0; b < grid; b++) ghz[b] = (double)h[2 * b] / (double)std::max<unsigned long long>(h[2 * b + 1], 1ull) * 0.1;      // s_memrealtime ticks at 100 MHz
    std::sort(ghz.begin(), ghz.end());
    const double clock = ghz[grid / 2];
    const double per_simd = (double)iters * kPerIter[MODE] * waves_per_simd;   // wave-instructions one SIMD issued (every SIMD holds waves_per_simd of the launch's waves)
    const double ns = ms * 1e6 / per_simd;
    std::fprintf(f, "%-46s %d waves/SIMD: %7.3f ms  %6.3f ns per wave-instruction per SIMD  clock %.2f GHz  -> %5.2f cycles\n", kNames[MODE], waves_per_simd, ms, ns, clock, ns * clock);
    hipFree(out); hipFree(cyc);
}
// EXEC modes (`valu exec`): what does a lane cost that is masked out of EXEC, against an active lane that computes on +inf?  The walk's
// own statements -- EV_VISIT_TEXT (scalar box operands, the walk's op_sel patterns, the descent decision behind it) and EV_PAIR_TEXT, from
// device_common.hpp, on the walk's temporaries v[52:63] -- at eight waves per SIMD, in five arms:
//   a  EXEC full, finite data in every lane
//   b  EXEC full, +inf origin terms in a fixed 60 % of the lanes (lane % 5 < 3: what an occluded lane used to carry; the pair test reads no
//      origin term, so for it b is a)
//   c  the same 60 % masked out of EXEC
//   d  EXEC = lanes 0-31        e  EXEC = lanes 32-63       (does the part skip a half of a wave64 that is all inactive?)
// Every arm runs the same instruction stream: each statement opens with s_mov_b64 exec, mask and ends with s_mov_b64 exec, -1 (mask = -1 in
// a and b).  Reported as above: ns per vector wave-instruction per SIMD by events, the clock held inside the loop, cycles.
struct ExecOps { v2f q[12]; float tmin, tmax; };
enum { MIX_NODE, MIX_PAIR };
template <int MIX> __attribute__((amdgpu_num_vgpr(50))) __global__ __launch_bounds__(256) void kexec(float *out, unsigned long long *cyc, ExecOps ops, int arm, int iters) {
    const int lane = threadIdx.x & 63;
    const bool dead = lane % 5 < 3;
    const unsigned long long mask = arm == 2 ? __builtin_amdgcn_ballot_w64(!dead) : arm == 3 ? 0xffffffffull : arm == 4 ? 0xffffffff00000000ull : ~0ull;
    // a ray per lane: directions that differ from lane to lane, a shared origin
    const float dx = 0.3f + 0.011f * lane, dy = 0.9f - 0.007f * lane, dz = -0.4f - 0.003f * lane, ox = 0.25f, oy = -0.5f, oz = 0.75f;
    const float inf = __builtin_inff();
    const bool infl = arm == 1 && dead;
    v2f pa_ = { 1.0f / dx, 1.0f / dy }, pb_ = { 1.0f / dz, fabsf(1.0f / dx) }, pc_ = { fabsf(1.0f / dy), fabsf(1.0f / dz) };
    v2f pd_ = { infl ? inf : -ox / dx, infl ? inf : -oy / dy }, pe_ = { infl ? inf : -oz / dz, infl ? inf : -oz / dz };
    v2f ra_ = { dx, dy }, rb_ = { dz, ox }, rc_ = { oy, oz };
    asm volatile("" : "+v"(rc_));
    int vstack = 0, acc = 0;
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (MIX == MIX_NODE) {
                unsigned long long m1_, t64_; int p0_, p1_, cur = 0, sp = 0;
#define UB_NODE(T0, T1, T2, T3, T4, T5, T0L, T0H, T1L, T1H, T2L, T2H, T3L, T3H, T4L, T4H, T5L, T5H)                                             \
                asm volatile("s_mov_b64 exec, %[mask]\n\t"                                                                                   \
                    EV_VISIT_TEXT("%[cx]", "%[cy]", "%[cz]", "%[hx]", "%[hy]", "%[hz]", "%[c0]", "%[c1]", "%[m1]", "%[t64]", "%[p0]", "%[p1]", \
                                  T0, T1, T2, T3, T4, T5, T0L, T0H, T1L, T1H, T2L, T2H, T3L, T3H, T4L, T4H, T5L, T5H)                        \
                    "s_mov_b64 exec, -1\n"                                                                                                   \
                    : [cur] "+s"(cur), [sp] "+s"(sp), [vstack] "+v"(vstack), [m1] "=&s"(m1_), [t64] "=&s"(t64_), [p0] "=&s"(p0_), [p1] "=&s"(p1_) \
                    : [cx] "s"(ops.q[0]), [cy] "s"(ops.q[1]), [cz] "s"(ops.q[2]), [hx] "s"(ops.q[3]), [hy] "s"(ops.q[4]), [hz] "s"(ops.q[5]), \
                      [c0] "s"(1 + u), [c1] "s"(9 + u), [pa] "v"(pa_), [pb] "v"(pb_), [pc] "v"(pc_), [pd] "v"(pd_), [pe] "v"(pe_), [mask] "s"(mask) \
                    : "vcc", "scc", "m0", T0L, T0H, T1L, T1H, T2L, T2H, T3L, T3H, T4L, T4H, T5L, T5H)
                EV_WITH(UB_NODE, EV_TMP_52);
#undef UB_NODE
                acc += cur;
            } else {
                unsigned long long ha, hb;
#define UB_PAIR(T0, T1, T2, T3, T4, T5, T0L, T0H, T1L, T1H, T2L, T2H, T3L, T3H, T4L, T4H, T5L, T5H)                                             \
                asm volatile("s_mov_b64 exec, %[mask]\n\t"                                                                                   \
                    EV_PAIR_TEXT("%[p0x]", "%[p0y]", "%[p0z]", "%[e0x]", "%[e0y]", "%[e0z]", "%[e1x]", "%[e1y]", "%[e1z]", "%[nx]", "%[ny]", "%[nz]", \
                                 "%[ha]", "%[hb]", T0, T1, T2, T3, T4, T5, T0L, T0H, T1L, T1H, T2L, T2H, T3L, T3H, T4L, T4H, T5L, T5H)       \
                    "s_mov_b64 exec, -1\n"                                                                                                   \
                    : [ha] "=&s"(ha), [hb] "=&s"(hb)                                                                                         \
                    : [p0x] "s"(ops.q[0]), [p0y] "s"(ops.q[1]), [p0z] "s"(ops.q[2]), [e0x] "s"(ops.q[3]), [e0y] "s"(ops.q[4]), [e0z] "s"(ops.q[5]), \
                      [e1x] "s"(ops.q[6]), [e1y] "s"(ops.q[7]), [e1z] "s"(ops.q[8]), [nx] "s"(ops.q[9]), [ny] "s"(ops.q[10]), [nz] "s"(ops.q[11]), \
                      [ra] "v"(ra_), [rb] "v"(rb_), [rc] "v"(rc_), [tmin] "s"(ops.tmin), [tmax] "s"(ops.tmax), [mask] "s"(mask)              \
                    : "vcc", "scc", T0L, T0H, T1L, T1H, T2L, T2H, T3L, T3H, T4L, T4H, T5L, T5H)
                EV_WITH(UB_PAIR, EV_TMP_52);
#undef UB_PAIR
                acc += (int)(ha & 1ull) + (int)(hb & 1ull);
            }
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
    out[blockIdx.x * 256 + threadIdx.x] = (float)(acc + vstack);
    if (threadIdx.x == 0) { cyc[2 * blockIdx.x] = t1 - t0; cyc[2 * blockIdx.x + 1] = r1 - r0; }
}
template <int MIX> void run_exec(FILE *f) {
    const int waves_per_simd = 8, grid = 256 * waves_per_simd, iters = 4000, per_iter = 4 * (MIX == MIX_NODE ? 15 : 40);
    // the node: two boxes about the rays (centres x x y y z z, half-sizes x x y y z z); the pair: two triangles of a leaf (p0, e0, e1, n)
    ExecOps ops = {};
    const float node[12] = { 0.5f, 0.75f, 0.5f, 0.25f, 0.5f, 0.625f, 0.25f, 0.125f, 0.5f, 0.25f, 0.25f, 0.375f };
    const float pair[24] = { 0.5f, 0.75f, 0.25f, 0.5f, 0.0f, 0.125f, 0.25f, -0.25f, 0.0f, 0.375f, 0.125f, 0.0f,
                             0.0f, 0.125f, -0.25f, -0.25f, 0.125f, -0.125f, 0.03125f, 0.0625f, 0.03125f, -0.03125f, -0.0625f, 0.125f };
    for (int k = 0; k < 12; k++) { ops.q[k].x = MIX == MIX_NODE ? (k < 6 ? node[2 * k] : 0.0f) : pair[2 * k]; ops.q[k].y = MIX == MIX_NODE ? (k < 6 ? node[2 * k + 1] : 0.0f) : pair[2 * k + 1]; }
    ops.tmin = 0.0001f; ops.tmax = 1.0f - 0.0001f;
    float *out; unsigned long long *cyc;
    hipMalloc(&out, (size_t)grid * 256 * 4); hipMalloc(&cyc, (size_t)grid * 16);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const char *arms[5] = { "a EXEC full, finite", "b EXEC full, 60 % +inf", "c 60 % out of EXEC", "d EXEC = lanes 0-31", "e EXEC = lanes 32-63" };
    for (int rep = 0; rep < 2; rep++)          // every arm twice, interleaved: the second pass shows what a repeat is worth
        for (int arm = 0; arm < 5; arm++) {
            kexec<MIX><<<grid, 256>>>(out, cyc, ops, arm, 10);
            hipEventRecord(e0); kexec<MIX><<<grid, 256>>>(out, cyc, ops, arm, iters); hipEventRecord(e1); hipEventSynchronize(e1);
            float ms; hipEventElapsedTime(&ms, e0, e1);
            std::vector<unsigned long long> h((size_t)grid * 2); hipMemcpy(h.data(), cyc, (size_t)grid * 16, hipMemcpyDeviceToHost);
            std::vector<double> ghz((size_t)grid);
            for (int b = 0; b < grid; b++) ghz[b] = (double)h[2 * b] / (double)std::max<unsigned long long>(h[2 * b + 1], 1ull) * 0.1;
            std::sort(ghz.begin(), ghz.end());
            const double clock = ghz[grid / 2], ns = ms * 1e6 / ((double)iters * per_iter * waves_per_simd);
            std::fprintf(f, "%-34s %-24s %7.3f ms  %6.3f ns per wave-instruction per SIMD  clock %.2f GHz  -> %5.2f cycles\n",
                         MIX == MIX_NODE ? "node visit (9 pk_fma 4 max3/min3 2 cmp)" : "pair test (40 vector instructions)", arms[arm], ms, ns, clock, ns * clock);
        }
    std::fprintf(f, "\n");
    hipFree(out); hipFree(cyc);
}
template <int M> void all(FILE *f) { for (int w : { 1, 2, 4, 8 }) run<M>(w, f); std::fprintf(f, "\n"); }
int main(int argc, char **argv) {
    FILE *f = stdout;
    hipDeviceProp_t pr; hipGetDeviceProperties(&pr, 0);
    std::fprintf(f, "# %s, %d CUs, clockRate %d kHz; 256-thread workgroups, one per CU per wave-per-SIMD step; eight independent registers per lane\n", pr.gcnArchName, pr.multiProcessorCount, pr.clockRate);
    if (argc > 1 && std::string(argv[1]) == "exec") { run_exec<MIX_NODE>(f); run_exec<MIX_PAIR>(f); return 0; }
    if (argc > 1 && std::string(argv[1]) == "lanemoves") { all<READFIRSTLANE>(f); all<READLANE>(f); all<PK_FMA_OPSEL>(f); return 0; }      // (the packed fma beside them: same run, same clock regime)
    all<FMA>(f); all<PK_FMA>(f); all<PK_FMA_OPSEL>(f); all<PK_MUL>(f); all<MAX3>(f); all<MAX3_CLAMP>(f); all<CMP_VCC>(f); all<CMP_SGPR>(f);
    all<EXP>(f); all<LOG>(f); all<RCP>(f); all<MOV>(f); all<WRITELANE>(f); all<MIX_VISIT>(f);
    all<MUL_LO_U32>(f); all<MAD_U64_U32>(f); all<MUL_F32>(f); all<SQRT>(f); all<SIN>(f); all<ALIGNBIT>(f);
    all<READFIRSTLANE>(f); all<READLANE>(f);
    return 0;
}
