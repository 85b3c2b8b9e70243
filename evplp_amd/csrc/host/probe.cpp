// Probe gather, host only (include/evplp.h "probe gather"): the term of one (record, point) pair in fp32 as probe_gather_kernel forms it,
// with IEEE division and square root and libm's powf where the kernel takes the hardware's rsq, rcp and exp2(e log2 d); the order-2 real
// spherical-harmonic basis; and the irradiance of a coefficient set on a surface.  No GPU, no context: what a caller's CPU path and the
// tests hold the kernel against.
#include "../../../include/evplp.h"

#include <cmath>

namespace {
constexpr float kInvPi = 0.318309886183790671537767526745028724068919291480912897495f;
constexpr float kPi = 3.14159265358979323846f;
inline float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }   // (the unit is built without contraction)
}

extern "C" void evplp_sh_basis(const float d[3], float y[9]) {
    const float x = d[0], yy = d[1], z = d[2];
    y[0] = 0.28209479f; y[1] = 0.48860251f * yy; y[2] = 0.48860251f * z; y[3] = 0.48860251f * x;
    y[4] = 1.09254843f * (x * yy); y[5] = 1.09254843f * (yy * z); y[6] = 0.31539157f * (3.0f * (z * z) - 1.0f);
    y[7] = 1.09254843f * (x * z); y[8] = 0.54627422f * (x * x - yy * yy);
}

extern "C" void evplp_probe_pair(const evplp_record *r, const float x[3], float min_distance, float out27[27]) {
    for (int i = 0; i < 27; i++) out27[i] = 0.0f;
    const float v12[3] = { r->pos[0] - x[0], r->pos[1] - x[1], r->pos[2] - x[2] };
    const float c2 = std::fmax(-dot3(r->normal, v12), 0.0f);
    if (!(c2 > 0.0f)) return;
    const float dist2 = dot3(v12, v12);
    if (!(dist2 >= 1.17549435e-38f && dist2 <= 3.4028235e38f)) return;         // not a normal finite number: no ray, no term (the kernel's test, on the same bits)
    const float inv_dist = 1.0f / std::sqrt(dist2);
    const float w[3] = { v12[0] * inv_dist, v12[1] * inv_dist, v12[2] * inv_dist };
    const float cos2 = c2 * inv_dist;
    float ph2 = 0.0f;
    if (r->rho_s[0] != 0.0f || r->rho_s[1] != 0.0f || r->rho_s[2] != 0.0f) {
        // PhongEvalF(-w, flux_dir, n, e): reflect(-flux_dir, n) = -flux_dir - 2 n (n . -flux_dir)
        const float in[3] = { -r->flux_dir[0], -r->flux_dir[1], -r->flux_dir[2] };
        const float nd = dot3(r->normal, in);
        const float refl[3] = { in[0] - (r->normal[0] * 2.0f) * nd, in[1] - (r->normal[1] * 2.0f) * nd, in[2] - (r->normal[2] * 2.0f) * nd };
        const float mw[3] = { -w[0], -w[1], -w[2] };
        const float d = std::fmax(dot3(mw, refl), 0.0f);
        if (d > 0.000001f) ph2 = (r->phong_exp + 2.0f) * (r->phong_exp == 0.0f ? 1.0f : powf(d, r->phong_exp)) * kInvPi * 0.5f;
    }
    const float g = cos2 / std::fmax(dist2, min_distance * min_distance);
    float E[3], y[9];
    for (int ch = 0; ch < 3; ch++) E[ch] = (r->flux[ch] * (r->rho_d[ch] * kInvPi + r->rho_s[ch] * ph2)) * g;
    evplp_sh_basis(w, y);
    for (int i = 0; i < 9; i++) for (int ch = 0; ch < 3; ch++) out27[3 * i + ch] = E[ch] * y[i];
}

extern "C" void evplp_sh_irradiance(const evplp_probe_sh *sh, const float normal[3], float rgb[3]) {
    const float a0 = kPi, a1 = 2.0f * kPi / 3.0f, a2 = kPi / 4.0f;      // the clamped cosine's band weights (Ramamoorthi and Hanrahan 2001)
    const float band[9] = { a0, a1, a1, a1, a2, a2, a2, a2, a2 };
    float y[9];
    evplp_sh_basis(normal, y);
    for (int ch = 0; ch < 3; ch++) {
        float s = 0.0f;
        for (int i = 0; i < 9; i++) s += (band[i] * y[i]) * sh->c[i][ch];
        rgb[ch] = s;
    }
}
