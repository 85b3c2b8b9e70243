// Surface gather, host only (include/evplp.h "surface gather"): the photon grid's plan, the cell of a position and the cell range of a
// point, exported from the header the kernels of kernels_surface.hip include (photon_grid.h).  No GPU, no context: the tests hold the
// range against the fp32 inside test with these.
#include "../../../include/evplp.h"
#include "../photon_grid.h"

extern "C" int evplp_photon_grid_plan(float radius, const float box_lo[3], const float box_hi[3], uint32_t usable_photons, float *edge, uint32_t *bits) {
    if (!box_lo || !box_hi || !edge || !bits) return EVPLP_ERR_INVALID;
    return pg_plan(radius, box_lo, box_hi, usable_photons, edge, bits) ? EVPLP_OK : EVPLP_ERR_INVALID;
}

extern "C" uint32_t evplp_photon_grid_cell(const float p[3], const float box_lo[3], float edge, uint32_t bits, int32_t cell[3]) {
    for (int k = 0; k < 3; k++) cell[k] = pg_cell1(p[k], box_lo[k], edge);
    return pg_bucket(cell[0], cell[1], cell[2], bits);
}

extern "C" int evplp_photon_grid_range(const float x[3], float radius, const float box_lo[3], const float box_hi[3], float edge, int32_t cell_lo[3], int32_t cell_hi[3]) {
    return pg_range(x, radius, box_lo, box_hi, edge, cell_lo, cell_hi);
}
