// The argument checks of include/nsdp_meshbatch.h as a stand-alone host program, in the manner of tools/batch_host_check.cpp: every
// refused call of nsdp_mesh_batch_sample (refused sizes, values that are not finite, null and misaligned pointers) returns before
// anything is launched, so the program needs no GPU -- which makes it the place for the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/meshbatch_host_check.cpp nsdp_amd/csrc/mesh_sample.hip nsdp_amd/csrc/api.hip -o meshbatch_host_check
//   ./meshbatch_host_check
//
// The pointers it passes are small integers the entry must never dereference; a read of one would be the sanitizer's report.
// Exit status 0 and "ok" when every call came back as expected.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/nsdp_hip.h"
#include "../include/nsdp_meshbatch.h"

namespace {

int failures = 0, calls = 0;

void expect(bool ok, const char *what) {
  ++calls;
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s (last error: %s)\n", what, nsdp_last_error());
    ++failures;
  }
}

bool refused_with(int rc, const char *word) {
  return rc == NSDP_EINVAL && std::strstr(nsdp_last_error(), word) != nullptr && std::strstr(nsdp_last_error(), "mesh_batch_sample") != nullptr;
}

template <class T>
T *fake(uintptr_t v) { return reinterpret_cast<T *>(v); }

struct Sample {
  const float *verts = fake<const float>(16);
  const int32_t *faces = fake<const int32_t>(32), *ids = fake<const int32_t>(16);
  const uint32_t *thr = fake<const uint32_t>(16);
  long long vert_rows = 10, face_rows = 10, thr_rows = 10;
  const int64_t *frames = fake<const int64_t>(16), *topos = fake<const int64_t>(24);
  int n_frames = 2, n_topos = 1, B = 2, n = 4, m = 4;
  float partial_range = 0.1f, sigma1 = 0.1f, sigma2 = 0.02f, noise_level = 0.f;
  const float *noise = nullptr;
  float *surface_out = fake<float>(16), *inputs_out = fake<float>(16), *space_out = fake<float>(16);
  uint8_t *handle_out = fake<uint8_t>(17);
  int call() const {
    return nsdp_mesh_batch_sample(verts, vert_rows, faces, face_rows, thr, thr_rows, frames, n_frames, topos, n_topos, ids, B, n, m,
                                  0x123456789ULL, 1u, 2u, partial_range, sigma1, sigma2, noise, noise_level, surface_out, handle_out,
                                  inputs_out, space_out, nullptr);
  }
};

}  // namespace

int main() {
  expect(nsdp_abi_version() >= 23, "ABI version 23");
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  char what[160];
  const struct { int B, n, m, n_frames, n_topos; long long vert_rows, face_rows, thr_rows; float range, s1, s2, level; const char *word; } table[] = {
      {-2, 4, 4, 2, 1, 10, 10, 10, 0.1f, 0.1f, 0.02f, 0.f, "B=-2"},
      {65536, 4, 4, 2, 1, 10, 10, 10, 0.1f, 0.1f, 0.02f, 0.f, "B=65536"},
      {2, -1, 4, 2, 1, 10, 10, 10, 0.1f, 0.1f, 0.02f, 0.f, "n=-1"},
      {2, 4, -1, 2, 1, 10, 10, 10, 0.1f, 0.1f, 0.02f, 0.f, "m=-1"},
      {2, (1 << 20) + 1, 4, 2, 1, 10, 10, 10, 0.1f, 0.1f, 0.02f, 0.f, "n=1048577"},
      {2, 4, (1 << 20) + 1, 2, 1, 10, 10, 10, 0.1f, 0.1f, 0.02f, 0.f, "m=1048577"},
      {1024, 1 << 17, 4, 2, 1, 10, 10, 10, 0.1f, 0.1f, 0.02f, 0.f, "too large"},
      {1024, 4, 1 << 17, 2, 1, 10, 10, 10, 0.1f, 0.1f, 0.02f, 0.f, "too large"},
      {2, 4, 4, 0, 1, 10, 10, 10, 0.1f, 0.1f, 0.02f, 0.f, "n_frames=0"},
      {2, 4, 4, 2, -1, 10, 10, 10, 0.1f, 0.1f, 0.02f, 0.f, "n_topos=-1"},
      {2, 4, 4, 2, 1, 0, 10, 10, 0.1f, 0.1f, 0.02f, 0.f, "vert_rows=0"},
      {2, 4, 4, 2, 1, 10, -4, 10, 0.1f, 0.1f, 0.02f, 0.f, "face_rows=-4"},
      {2, 4, 4, 2, 1, 10, 10, 0, 0.1f, 0.1f, 0.02f, 0.f, "thr_rows=0"},
      {2, 4, 4, 2, 1, 10, 10, 10, nan, 0.1f, 0.02f, 0.f, "partial_range"},
      {2, 4, 4, 2, 1, 10, 10, 10, 0.1f, inf, 0.02f, 0.f, "sigma"},
      {2, 4, 4, 2, 1, 10, 10, 10, 0.1f, 0.1f, nan, 0.f, "sigma"},
      {2, 4, 4, 2, 1, 10, 10, 10, 0.1f, 0.1f, 0.02f, -inf, "noise_level"}};
  for (const auto &row : table) {
    Sample s;
    s.B = row.B, s.n = row.n, s.m = row.m, s.n_frames = row.n_frames, s.n_topos = row.n_topos, s.vert_rows = row.vert_rows;
    s.face_rows = row.face_rows, s.thr_rows = row.thr_rows, s.partial_range = row.range, s.sigma1 = row.s1, s.sigma2 = row.s2;
    s.noise_level = row.level;
    std::snprintf(what, sizeof what, "mesh_batch_sample B=%d n=%d m=%d names '%s'", row.B, row.n, row.m, row.word);
    expect(refused_with(s.call(), row.word), what);
  }
  Sample sizes_first;      // sizes are judged before pointers
  sizes_first.n_frames = 0, sizes_first.frames = nullptr, sizes_first.ids = nullptr, sizes_first.verts = nullptr;
  expect(refused_with(sizes_first.call(), "n_frames=0"), "a refused size beside null pointers names the size");
  for (int which = 0; which < 10; ++which) {
    Sample s;
    if (which == 0) s.verts = nullptr;
    if (which == 1) s.faces = nullptr;
    if (which == 2) s.thr = nullptr;
    if (which == 3) s.frames = nullptr;
    if (which == 4) s.topos = nullptr;
    if (which == 5) s.ids = nullptr;
    if (which == 6) s.surface_out = nullptr;
    if (which == 7) s.handle_out = nullptr;
    if (which == 8) s.inputs_out = nullptr;
    if (which == 9) s.space_out = nullptr;
    expect(refused_with(s.call(), "null"), "a null pointer");
  }
  Sample a, b, c, d, e, f, g, h;
  a.verts = fake<const float>(24), b.faces = fake<const int32_t>(8), c.frames = fake<const int64_t>(20), d.topos = fake<const int64_t>(12);
  e.noise = fake<const float>(18), f.thr = fake<const uint32_t>(6);
  expect(refused_with(a.call(), "16-byte"), "a vertex arena that is not 16-byte aligned");
  expect(refused_with(b.call(), "16-byte"), "a face arena that is not 16-byte aligned");
  expect(refused_with(c.call(), "8-byte"), "a frame table that is not 8-byte aligned");
  expect(refused_with(d.call(), "8-byte"), "a topology table that is not 8-byte aligned");
  expect(refused_with(e.call(), "4-byte"), "misaligned noise");
  expect(refused_with(f.call(), "4-byte"), "misaligned thresholds");
  g.B = 0, g.frames = nullptr, g.ids = nullptr, g.verts = nullptr;
  expect(g.call() == 0, "B = 0 is nothing to do");
  h.n = 0, h.m = 0, h.frames = nullptr, h.verts = nullptr, h.faces = nullptr, h.thr = nullptr;
  expect(h.call() == 0, "n = m = 0 is nothing to do");
  // a part without rows may come without its outputs: the surviving refusal is the OTHER part's
  Sample no_surface;
  no_surface.n = 0, no_surface.surface_out = nullptr, no_surface.handle_out = nullptr, no_surface.inputs_out = nullptr, no_surface.space_out = nullptr;
  expect(refused_with(no_surface.call(), "space output"), "n = 0 leaves only the space output to refuse");
  if (failures) return 1;
  std::printf("ok: %d checks\n", calls);
  return 0;
}
