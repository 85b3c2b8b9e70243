// The planner of the path tracer's budget mode (include/evplp.h evplp_plan_budgets): host only, no device, nothing but the standard library,
// like the deal of row blocks (deal.cpp) -- every process of a multi-process run calls it for itself on the same figures and gets the same
// budgets.  Plain double arithmetic (this file is built without contraction): one product per tile for v_t, then one division, one sqrt,
// one product and one ceil.
#include "../../../include/evplp.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

extern "C" int evplp_plan_budgets(const double *rel, const int32_t *n_t, int32_t ntiles, int32_t samples, int32_t min_samples, double tile_rel_mse,
                                  double reference_quantile, int32_t *out_budgets) {
    if (!rel || !n_t || !out_budgets || ntiles < 1) return EVPLP_ERR_INVALID;
    if (samples < 1 || samples > 64 || min_samples < 0 || min_samples > samples) return EVPLP_ERR_INVALID;
    if (!(reference_quantile > 0.0) || !(reference_quantile <= 1.0)) return EVPLP_ERR_INVALID;
    for (int32_t t = 0; t < ntiles; t++) if (!std::isfinite(rel[t]) || rel[t] < 0.0) return EVPLP_ERR_INVALID;
    // v_t = rel_t * n_t: the relative variance of ONE sample of the tile (rel_t is that of the mean of n_t)
    std::vector<double> v((size_t)ntiles, 0.0), sorted;
    sorted.reserve((size_t)ntiles);
    for (int32_t t = 0; t < ntiles; t++)
        if (n_t[t] > 0) { v[(size_t)t] = rel[t] * (double)n_t[t]; sorted.push_back(v[(size_t)t]); }
    std::sort(sorted.begin(), sorted.end());
    const size_t m = sorted.size();
    const double v_ref = m ? sorted[std::min(m - 1, (size_t)std::floor(reference_quantile * (double)m))] : 0.0;
    const int32_t lo = std::max(1, min_samples);
    for (int32_t t = 0; t < ntiles; t++) {
        int32_t b;
        if (n_t[t] <= 0) b = 0;                                                     // not in the image, or nobody's
        else if (tile_rel_mse > 0.0 && rel[t] <= tile_rel_mse) b = 0;               // at the noise level asked for: the stopping rule
        else if (!(v_ref > 0.0)) b = samples;
        else {
            const double x = std::ceil((double)samples * std::sqrt(v[(size_t)t] / v_ref));
            b = !(x <= (double)samples) ? samples : x < (double)lo ? lo : (int32_t)x;
        }
        out_budgets[t] = b;
    }
    return EVPLP_OK;
}
