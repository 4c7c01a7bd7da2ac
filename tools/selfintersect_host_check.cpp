// The argument checks of include/nsdp_selfintersect.h as a stand-alone host program: every refused call of the bad-argument
// table (refused sizes, a negative budget, unknown flags, null and misaligned pointers) returns before anything is launched,
// so the program needs no GPU -- which makes it the place for the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/selfintersect_host_check.cpp nsdp_amd/csrc/self_intersect.hip nsdp_amd/csrc/api.hip -o selfintersect_host_check
//   ./selfintersect_host_check
//
// (tests/test_self_intersect_cpu.py links it against the built library instead, without a sanitizer.)  The pointers it passes
// are small integers the entry must never dereference; a read of one would be the sanitizer's report.  Exit status 0 and "ok"
// when every call came back as expected.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/nsdp_hip.h"
#include "../include/nsdp_selfintersect.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s (last error: %s)\n", what, nsdp_last_error());
    ++failures;
  }
}

bool refused_with(int rc, const char *word) {
  return rc == NSDP_EINVAL && std::strstr(nsdp_last_error(), word) != nullptr &&
         std::strstr(nsdp_last_error(), "mesh_self_intersections") != nullptr;
}

template <class T>
T *fake(uintptr_t v) { return reinterpret_cast<T *>(v); }

struct Args {
  const float *verts = fake<const float>(16);
  const int32_t *voff = fake<const int32_t>(16), *faces = fake<const int32_t>(16), *foff = fake<const int32_t>(16),
                *ids = fake<const int32_t>(16);
  int P = 1, B = 2, vcap = 8, fcap = 12, budget = 0, flags = 0;
  void *ws = fake<void>(16);
  int32_t *cand = fake<int32_t>(16), *hits = fake<int32_t>(16), *partner = fake<int32_t>(16), *skipped = fake<int32_t>(16);
  int64_t *pairs = fake<int64_t>(16);
  int call() const {
    return nsdp_mesh_self_intersections(verts, P, voff, faces, foff, ids, B, vcap, fcap, budget, flags, ws, cand, hits, partner, pairs,
                                        skipped, nullptr);
  }
};

}  // namespace

int main() {
  expect(nsdp_abi_version() >= 27, "ABI version 27");
  // the size query: 0 for what the entry refuses, else 4 P (10 fcap + 6 (fcap / 64 + B + 1))
  const auto size = nsdp_mesh_self_intersections_workspace_bytes;
  expect(size(0, 2, 12) == 0 && size(65536, 2, 12) == 0 && size(1, 0, 12) == 0 && size(1, 65536, 12) == 0 && size(1, 2, 0) == 0 &&
             size(1, -1, 12) == 0 && size(1, 1, 1048577) == 0 && size(-3, 1, 12) == 0,
         "size: refused sizes");
  expect(size(1, 2, 12) == 4u * (120u + 6u * 3u), "size: P=1 B=2 fcap=12");
  expect(size(3, 3, 129) == 12u * (1290u + 6u * 6u), "size: P=3 B=3 fcap=129");
  expect(size(1, 1, 1048576) == 4u * (10485760u + 6u * (16384u + 2u)), "size: the largest shape");

  char what[160];
  const struct { int P, B, vcap, fcap, budget, flags; const char *word; } table[] = {
      {0, 2, 8, 12, 0, 0, "P=0"},           {-1, 2, 8, 12, 0, 0, "P=-1"},         {65536, 2, 8, 12, 0, 0, "P=65536"},
      {1, 0, 8, 12, 0, 0, "B=0"},           {1, -2, 8, 12, 0, 0, "B=-2"},         {1, 65536, 8, 12, 0, 0, "B=65536"},
      {1, 2, 0, 12, 0, 0, "vcap=0"},        {1, 2, -5, 12, 0, 0, "vcap=-5"},      {1, 1, 1048577, 12, 0, 0, "vcap=1048577"},
      {1, 2, 8, 0, 0, 0, "fcap=0"},         {1, 2, 8, -1, 0, 0, "fcap=-1"},       {1, 1, 8, 1048577, 0, 0, "fcap=1048577"},
      {1, 2, 8, 12, -1, 0, "budget=-1"},    {1, 2, 8, 12, 0, 2, "flags=2"},       {1, 2, 8, 12, 0, -1, "flags=-1"},
      {1, 2, 8, 12, 0, 4, "flags=4"},       {0, 0, 0, 0, -1, 8, "P=0"},           {1, 2, 8, 0, -1, 8, "fcap=0"},
      {1, 2, 8, 12, -7, 8, "budget=-7"}};
  for (const auto &row : table) {
    Args a;
    a.P = row.P, a.B = row.B, a.vcap = row.vcap, a.fcap = row.fcap, a.budget = row.budget, a.flags = row.flags;
    std::snprintf(what, sizeof what, "P=%d B=%d vcap=%d fcap=%d budget=%d flags=%d names '%s'", row.P, row.B, row.vcap, row.fcap,
                  row.budget, row.flags, row.word);
    expect(refused_with(a.call(), row.word), what);
  }
  {
    Args a;      // sizes are judged before pointers
    a.verts = nullptr, a.voff = a.faces = a.foff = nullptr, a.ws = nullptr, a.cand = a.hits = a.partner = a.skipped = nullptr, a.pairs = nullptr;
    a.fcap = 0;
    expect(refused_with(a.call(), "fcap=0"), "a refused size beside null pointers names the size");
    Args b;      // (the largest shape is a size the entry takes: the pointer is named)
    b.B = 1, b.vcap = b.fcap = 1048576, b.P = 65535, b.verts = nullptr;
    expect(refused_with(b.call(), "null"), "the largest shape beside a null pointer names the pointer");
  }
  for (int which = 0; which < 10; ++which) {
    Args a;
    if (which == 0) a.verts = nullptr;
    if (which == 1) a.voff = nullptr;
    if (which == 2) a.faces = nullptr;
    if (which == 3) a.foff = nullptr;
    if (which == 4) a.ws = nullptr;
    if (which == 5) a.cand = nullptr;
    if (which == 6) a.hits = nullptr;
    if (which == 7) a.partner = nullptr;
    if (which == 8) a.pairs = nullptr;
    if (which == 9) a.skipped = nullptr;
    expect(refused_with(a.call(), "null"), "a null pointer");
  }
  {
    Args a;      // pointers before alignment
    a.ws = fake<void>(24), a.hits = nullptr;
    expect(refused_with(a.call(), "null"), "a null pointer beside a misaligned one names the null");
    Args b;
    b.ws = fake<void>(24);
    expect(refused_with(b.call(), "16-byte"), "a workspace that is not 16-byte aligned");
    for (int which = 0; which < 9; ++which) {
      Args c;
      if (which == 0) c.verts = fake<const float>(18);
      if (which == 1) c.voff = fake<const int32_t>(18);
      if (which == 2) c.faces = fake<const int32_t>(18);
      if (which == 3) c.foff = fake<const int32_t>(18);
      if (which == 4) c.ids = fake<const int32_t>(18);
      if (which == 5) c.cand = fake<int32_t>(18);
      if (which == 6) c.hits = fake<int32_t>(18);
      if (which == 7) c.partner = fake<int32_t>(18);
      if (which == 8) c.skipped = fake<int32_t>(18);
      expect(refused_with(c.call(), "4-byte"), "an operand that is not 4-byte aligned");
    }
    Args d;
    d.pairs = fake<int64_t>(20);
    expect(refused_with(d.call(), "8-byte"), "pairs_out that is not 8-byte aligned");
  }
  if (failures) return 1;
  std::puts("ok");
  return 0;
}
