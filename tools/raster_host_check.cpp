// The argument checks of include/nsdp_raster.h as a stand-alone host program: every refused call of the bad-argument table
// (refused sizes, unknown flags, null and misaligned pointers) returns before anything is launched, so the program needs no
// GPU -- which makes it the place for the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/raster_host_check.cpp nsdp_amd/csrc/rasterize.hip nsdp_amd/csrc/api.hip -o raster_host_check
//   ./raster_host_check
//
// The pointers it passes are small integers the entry must never dereference; a read of one would be the sanitizer's report.
// Exit status 0 and "ok" when every call came back as expected.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/nsdp_hip.h"
#include "../include/nsdp_raster.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s (last error: %s)\n", what, nsdp_last_error());
    ++failures;
  }
}

bool refused_with(int rc, const char *word) {
  return rc == NSDP_EINVAL && std::strstr(nsdp_last_error(), word) != nullptr && std::strstr(nsdp_last_error(), "mesh_rasterize") != nullptr;
}

template <class T>
T *fake(uintptr_t v) { return reinterpret_cast<T *>(v); }

struct Args {
  const float *verts = fake<const float>(16), *cams = fake<const float>(16);
  const int32_t *voff = fake<const int32_t>(16), *faces = fake<const int32_t>(16), *foff = fake<const int32_t>(16),
                *shape = fake<const int32_t>(16);
  int B = 2, I = 3, vcap = 8, fcap = 12, H = 33, W = 17, flags = 0;
  void *ws = fake<void>(16);
  float *depth = fake<float>(16), *bary = fake<float>(16);
  int32_t *face = fake<int32_t>(16), *count = fake<int32_t>(16), *dropped = fake<int32_t>(16);
  int call() const {
    return nsdp_mesh_rasterize(verts, voff, faces, foff, cams, shape, B, I, vcap, fcap, H, W, flags, ws, depth, face, bary, count,
                               dropped, nullptr);
  }
};

}  // namespace

int main() {
  expect(nsdp_abi_version() >= 30, "ABI version 30");
  // the size query: 0 for what the entry refuses, 20 bytes per image and box slot (fcap / 64 + B + 1) otherwise
  expect(nsdp_mesh_rasterize_workspace_bytes(0, 3, 12) == 0 && nsdp_mesh_rasterize_workspace_bytes(65536, 3, 12) == 0 &&
             nsdp_mesh_rasterize_workspace_bytes(2, 0, 12) == 0 && nsdp_mesh_rasterize_workspace_bytes(2, 65536, 12) == 0 &&
             nsdp_mesh_rasterize_workspace_bytes(2, 3, 0) == 0 && nsdp_mesh_rasterize_workspace_bytes(-1, 3, 12) == 0 &&
             nsdp_mesh_rasterize_workspace_bytes(2, -3, 12) == 0 && nsdp_mesh_rasterize_workspace_bytes(1, 3, 1048577) == 0,
         "size: refused sizes");
  expect(nsdp_mesh_rasterize_workspace_bytes(2, 3, 12) == 20u * 3u * 3u, "size: B=2 I=3 fcap=12");
  expect(nsdp_mesh_rasterize_workspace_bytes(1, 1, 1048576) == 20u * (16384u + 2u), "size: the largest shape");
  expect(nsdp_mesh_rasterize_workspace_bytes(3, 5, 129) == 20u * 5u * 6u, "size: B=3 I=5 fcap=129");
  expect(nsdp_mesh_rasterize_workspace_bytes(65535, 65535, 2147483647) == static_cast<size_t>(20) * 65535u * (33554431u + 65536u),
         "size: beyond 2^32 bytes");

  char what[160];
  const struct { int B, I, vcap, fcap, H, W, flags; const char *word; } table[] = {
      {0, 3, 8, 12, 33, 17, 0, "B=0"},          {-2, 3, 8, 12, 33, 17, 0, "B=-2"},         {65536, 3, 8, 12, 33, 17, 0, "B=65536"},
      {2, 0, 8, 12, 33, 17, 0, "I=0"},          {2, -1, 8, 12, 33, 17, 0, "I=-1"},         {2, 65536, 8, 12, 33, 17, 0, "I=65536"},
      {2, 3, 0, 12, 33, 17, 0, "vcap=0"},       {2, 3, -5, 12, 33, 17, 0, "vcap=-5"},      {1, 3, 1048577, 12, 33, 17, 0, "vcap=1048577"},
      {2, 3, 8, 0, 33, 17, 0, "fcap=0"},        {2, 3, 8, -1, 33, 17, 0, "fcap=-1"},       {1, 3, 8, 1048577, 33, 17, 0, "fcap=1048577"},
      {2, 3, 8, 12, 0, 17, 0, "H=0"},           {2, 3, 8, 12, 4097, 17, 0, "H=4097"},      {2, 3, 8, 12, -33, 17, 0, "H=-33"},
      {2, 3, 8, 12, 33, 0, 0, "W=0"},           {2, 3, 8, 12, 33, 4097, 0, "W=4097"},      {2, 3, 8, 12, 33, -1, 0, "W=-1"},
      {2, 128, 8, 12, 4096, 4096, 0, "2^31"},   {2, 32768, 8, 12, 256, 256, 0, "2^31"},
      {2, 3, 8, 12, 33, 17, 2, "flags=2"},      {2, 3, 8, 12, 33, 17, -1, "flags=-1"},     {2, 3, 8, 12, 33, 17, 3, "flags=3"}};
  for (const auto &row : table) {
    Args a;
    a.B = row.B, a.I = row.I, a.vcap = row.vcap, a.fcap = row.fcap, a.H = row.H, a.W = row.W, a.flags = row.flags;
    std::snprintf(what, sizeof what, "B=%d I=%d vcap=%d fcap=%d H=%d W=%d flags=%d names '%s'", row.B, row.I, row.vcap, row.fcap, row.H,
                  row.W, row.flags, row.word);
    expect(refused_with(a.call(), row.word), what);
  }
  {
    Args a;      // sizes are judged before pointers
    a.verts = a.cams = nullptr, a.voff = a.faces = a.foff = a.shape = nullptr, a.ws = nullptr, a.depth = nullptr, a.face = nullptr;
    a.W = 0;
    expect(refused_with(a.call(), "W=0"), "a refused size beside null pointers names the size");
    Args b;      // (the largest image count below 2^31 pixels is a size the entry takes: the pointer is named)
    b.I = 127, b.H = b.W = 4096, b.verts = nullptr;
    expect(refused_with(b.call(), "null"), "the largest images beside a null pointer name the pointer");
    Args c;      // flags are judged before pointers
    c.flags = 2, c.cams = nullptr;
    expect(refused_with(c.call(), "flags=2"), "unknown flags beside a null pointer name the flags");
  }
  for (int which = 0; which < 10; ++which) {
    Args a;
    if (which == 0) a.verts = nullptr;
    if (which == 1) a.voff = nullptr;
    if (which == 2) a.faces = nullptr;
    if (which == 3) a.foff = nullptr;
    if (which == 4) a.cams = nullptr;
    if (which == 5) a.shape = nullptr;
    if (which == 6) a.ws = nullptr;
    if (which == 7) a.depth = nullptr;
    if (which == 8) a.face = nullptr;
    if (which == 9) a.dropped = nullptr;
    expect(refused_with(a.call(), "null"), "a null pointer");
  }
  {
    Args a;      // pointers are judged before the alignment
    a.ws = fake<void>(24);
    expect(refused_with(a.call(), "aligned"), "a workspace that is not 16-byte aligned");
    a.dropped = nullptr;
    expect(refused_with(a.call(), "null"), "a null pointer beside a misaligned workspace names the pointer");
  }
  if (failures) return 1;
  std::puts("ok");
  return 0;
}
