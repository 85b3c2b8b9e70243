// host/skin.cpp: what evplp_set_mesh_skin, evplp_pose_mesh and evplp_skin_points refuse about their arrays, and the one loop that moves points
// through skin_point (evplp_types.h).  Host only: no device, no context.
#pragma once
#include <cstddef>
#include <cstdint>

namespace evplp {
// a skin of nverts vertices over nbones bones (int32[nverts][4], float[nverts][4]): false and the reason in why for a null pointer, nbones
// outside 1 .. 1024, nverts < 0, an index outside [0, nbones) (also where its weight is 0), a weight that is not finite or is negative, a
// vertex whose four weights, added in double, differ from 1 by more than 1e-3
bool skin_arrays_ok(int32_t nbones, const int32_t *bone_index, const float *weight, int32_t nverts, char *why, size_t cap);
// a palette of nbones row-major 3 x 4 matrices: false for a null pointer or an entry that is not finite
bool skin_palette_ok(const float *bone_matrices, int32_t nbones, char *why, size_t cap);
// out[v] = skin_point(in[v]) for n points (float3 each; out may be in).  Returns the first point with a coordinate that is not finite, -1: none
// (every point is written either way)
int64_t skin_apply(const float *bone_matrices, const int32_t *bone_index, const float *weight, const float *in, float *out, size_t n);
}
