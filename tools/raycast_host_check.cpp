// The argument checks of include/nsdp_raycast.h as a stand-alone host program: every refused call of the bad-argument table
// (refused sizes, unknown flags, null and misaligned pointers) returns before anything is launched, so the program needs no
// GPU -- which makes it the place for the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/raycast_host_check.cpp nsdp_amd/csrc/ray_cast.hip nsdp_amd/csrc/api.hip -o raycast_host_check
//   ./raycast_host_check
//
// The pointers it passes are small integers the entry must never dereference; a read of one would be the sanitizer's report.
// Exit status 0 and "ok" when every call came back as expected.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/nsdp_hip.h"
#include "../include/nsdp_raycast.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s (last error: %s)\n", what, nsdp_last_error());
    ++failures;
  }
}

bool refused_with(int rc, const char *word) {
  return rc == NSDP_EINVAL && std::strstr(nsdp_last_error(), word) != nullptr && std::strstr(nsdp_last_error(), "mesh_ray_cast") != nullptr;
}

template <class T>
T *fake(uintptr_t v) { return reinterpret_cast<T *>(v); }

struct Args {
  const float *origins = fake<const float>(16), *dirs = fake<const float>(16), *verts = fake<const float>(16);
  const int32_t *roff = fake<const int32_t>(16), *voff = fake<const int32_t>(16), *faces = fake<const int32_t>(16),
                *foff = fake<const int32_t>(16);
  int B = 2, qcap = 10, vcap = 8, fcap = 12, flags = 0;
  void *ws = fake<void>(16);
  float *t = fake<float>(16), *bary = fake<float>(16);
  int32_t *face = fake<int32_t>(16), *count = fake<int32_t>(16);
  int call() const {
    return nsdp_mesh_ray_cast(origins, dirs, roff, verts, voff, faces, foff, B, qcap, vcap, fcap, flags, ws, t, face, bary, count,
                              nullptr);
  }
};

}  // namespace

int main() {
  expect(nsdp_abi_version() >= 28, "ABI version 28");
  // the size query: 0 for what the entry refuses, 12 bytes per ray row + 24 per box slot (fcap / 64 + B + 1) otherwise
  expect(nsdp_mesh_ray_cast_workspace_bytes(0, 10, 12) == 0 && nsdp_mesh_ray_cast_workspace_bytes(65536, 10, 12) == 0 &&
             nsdp_mesh_ray_cast_workspace_bytes(2, 0, 12) == 0 && nsdp_mesh_ray_cast_workspace_bytes(2, 10, 0) == 0 &&
             nsdp_mesh_ray_cast_workspace_bytes(-1, 10, 12) == 0 && nsdp_mesh_ray_cast_workspace_bytes(1, 1048577, 12) == 0 &&
             nsdp_mesh_ray_cast_workspace_bytes(1, 10, 1048577) == 0,
         "size: refused sizes");
  expect(nsdp_mesh_ray_cast_workspace_bytes(2, 10, 12) == 12u * 10u + 24u * 3u, "size: B=2 qcap=10 fcap=12");
  expect(nsdp_mesh_ray_cast_workspace_bytes(1, 1048576, 1048576) == 12u * 1048576u + 24u * (16384u + 2u), "size: the largest shape");
  expect(nsdp_mesh_ray_cast_workspace_bytes(3, 1, 129) == 12u + 24u * 6u, "size: B=3 qcap=1 fcap=129");

  char what[128];
  const struct { int B, qcap, vcap, fcap, flags; const char *word; } table[] = {
      {0, 10, 8, 12, 0, "B=0"},         {-2, 10, 8, 12, 0, "B=-2"},        {65536, 10, 8, 12, 0, "B=65536"},
      {2, 0, 8, 12, 0, "qcap=0"},       {2, -1, 8, 12, 0, "qcap=-1"},      {2, 2097153, 8, 12, 0, "qcap=2097153"},
      {2, 10, 0, 12, 0, "vcap=0"},      {2, 10, -5, 12, 0, "vcap=-5"},     {1, 10, 1048577, 12, 0, "vcap=1048577"},
      {2, 10, 8, 0, 0, "fcap=0"},       {2, 10, 8, -1, 0, "fcap=-1"},      {1, 10, 8, 1048577, 0, "fcap=1048577"},
      {2, 10, 8, 12, 2, "flags=2"},     {2, 10, 8, 12, -1, "flags=-1"},    {2, 10, 8, 12, 3, "flags=3"}};
  for (const auto &row : table) {
    Args a;
    a.B = row.B, a.qcap = row.qcap, a.vcap = row.vcap, a.fcap = row.fcap, a.flags = row.flags;
    std::snprintf(what, sizeof what, "B=%d qcap=%d vcap=%d fcap=%d flags=%d names '%s'", row.B, row.qcap, row.vcap, row.fcap, row.flags,
                  row.word);
    expect(refused_with(a.call(), row.word), what);
  }
  {
    Args a;      // sizes are judged before pointers
    a.origins = a.dirs = a.verts = nullptr, a.roff = a.voff = a.faces = a.foff = nullptr, a.ws = nullptr, a.t = nullptr, a.face = nullptr;
    a.fcap = 0;
    expect(refused_with(a.call(), "fcap=0"), "a refused size beside null pointers names the size");
    Args b;      // (the largest shape is a size the entry takes: the pointer is named)
    b.B = 1, b.qcap = b.vcap = b.fcap = 1048576, b.origins = nullptr;
    expect(refused_with(b.call(), "null"), "the largest shape beside a null pointer names the pointer");
    Args c;      // flags are judged before pointers
    c.flags = 2, c.dirs = nullptr;
    expect(refused_with(c.call(), "flags=2"), "unknown flags beside a null pointer name the flags");
  }
  for (int which = 0; which < 10; ++which) {
    Args a;
    if (which == 0) a.origins = nullptr;
    if (which == 1) a.dirs = nullptr;
    if (which == 2) a.roff = nullptr;
    if (which == 3) a.verts = nullptr;
    if (which == 4) a.voff = nullptr;
    if (which == 5) a.faces = nullptr;
    if (which == 6) a.foff = nullptr;
    if (which == 7) a.ws = nullptr;
    if (which == 8) a.t = nullptr;
    if (which == 9) a.face = nullptr;
    expect(refused_with(a.call(), "null"), "a null pointer");
  }
  {
    Args a;      // pointers are judged before the alignment
    a.ws = fake<void>(20);
    expect(refused_with(a.call(), "aligned"), "a workspace that is not 8-byte aligned");
    a.face = nullptr;
    expect(refused_with(a.call(), "null"), "a null pointer beside a misaligned workspace names the pointer");
  }
  if (failures) return 1;
  std::puts("ok");
  return 0;
}
