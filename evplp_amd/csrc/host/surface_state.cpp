// Progressive surface gather, host only (include/evplp.h "progressive surface gather"): a point's state through one photon half, and its
// resolve, exported from the header the kernels of kernels_surface_prog.hip include (surface_state.h).  No GPU, no context: the tests
// hold the rule against a numpy float32 restatement, bit for bit, with these.
#include "../../../include/evplp.h"
#include "../surface_state.h"

extern "C" int evplp_surface_state_update(evplp_surface_state *state, uint32_t m, const float phi[3], float alpha, float r0sq) {
    if (!state || !phi) return EVPLP_ERR_INVALID;
    // (the kernel's decision, before it walks: a state whose radius2 is out of range is flagged and nothing else of it changes)
    if (!ss_radius_ok(state->pm_calls, state->radius2, r0sq)) { state->flags |= EVPLP_STATE_INVALID; return EVPLP_OK; }
    ss_update(state, m, phi, alpha, r0sq);
    return EVPLP_OK;
}

extern "C" int evplp_surface_state_resolve(const evplp_surface_state *state, evplp_surface_light *out) {
    if (!state || !out) return EVPLP_ERR_INVALID;
    ss_resolve(state, out);
    return EVPLP_OK;
}
