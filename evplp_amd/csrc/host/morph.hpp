// host/morph.cpp: what evplp_set_mesh_morph, evplp_morph_mesh and evplp_morph_points refuse about their arrays, the one loop that moves points
// through morph_point (evplp_types.h), and the loop that puts a morphed base under the matrix or the pose in force.  Host only: no device, no context.
#pragma once
#include <cstddef>
#include <cstdint>

namespace evplp {
// ntargets targets of nverts vertices (float[ntargets][nverts][3]): false and the reason in why for ntargets outside 1 .. 64, nverts < 0, a null
// pointer, a delta that is not finite
bool morph_deltas_ok(int32_t ntargets, const float *deltas, int32_t nverts, char *why, size_t cap);
// ntargets weights: false for a null pointer or a weight that is not finite (any finite value is legal)
bool morph_weights_ok(const float *weights, int32_t ntargets, char *why, size_t cap);
// out[v] = morph_point(in[v]) under deltas[ntargets][n][3] and the weights, for n points (float3 each; out may be in).  Returns the first point
// with a coordinate that is not finite, -1: none (every point is written either way)
int64_t morph_apply(const float *deltas, const float *weights, int32_t ntargets, const float *in, float *out, size_t n);
// the positions of a mesh from its base (the morphed rest pose, or the rest pose): morphed first, then moved -- by the matrix (transform_point)
// where matrix is not null, by the palette over the skin (skin_point) where palette is not null, copied otherwise.  out may not be base.  Returns
// the first vertex with a coordinate that is not finite, -1: none
int64_t morph_deform(const float *base, const float *matrix, const float *palette, const int32_t *bone_index, const float *bone_weight, float *out, size_t n);
}
