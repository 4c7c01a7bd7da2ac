// The corners of a packed mesh, once: which packed vertex row a corner c = 3 q + j names (include/nsdp_meshnormals.h, "Corners").
// Shared by mesh_normals.hip (the corner lists, the face normals) and geodesic.hip (the edge table over the same lists), so both
// clamp a stale index by one text.
#pragma once

#include "packed_rows.h"      // a row's owner

namespace {

struct Mesh {
  const int32_t *faces, *face_offsets, *vert_offsets;
  int B, vcap, fcap;
};

// the packed vertex rows the corners of face row q of shape b name
__device__ __forceinline__ void corner_rows_of(const Mesh &m, long long q, int b, int rows[3]) {
  int first, end;
  shape_range(m.vert_offsets, b, m.vcap, first, end);
  const int hi = max(end - first - 1, 0);
  const int32_t *f = m.faces + static_cast<size_t>(q) * 3;
#pragma unroll
  for (int j = 0; j < 3; ++j) rows[j] = min(first + clamped(f[j], 0, hi), m.vcap - 1);
}

// the packed vertex rows the corners of face row q < fcap name, for lanes that hold ASCENDING face rows (one owner search per
// wave); false: a dead face (rows untouched)
__device__ __forceinline__ bool corner_rows(const Mesh &m, long long q, int rows[3]) {
  int b;
  if (!owner_of_lane(m.face_offsets, m.B, m.fcap, q, b)) return false;
  corner_rows_of(m, q, b, rows);
  return true;
}

// the same for a lane whose face row has nothing to do with its neighbours' (a search per lane)
__device__ __forceinline__ bool corner_rows_any(const Mesh &m, int q, int rows[3]) {
  int b, first, end;
  if (!owner_of(m.face_offsets, m.B, m.fcap, q, b, first, end)) return false;
  corner_rows_of(m, q, b, rows);
  return true;
}

}  // namespace
