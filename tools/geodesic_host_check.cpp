// The argument checks of include/nsdp_geodesic.h as a stand-alone host program: every refused call of the bad-argument table
// (refused sizes, a NaN or negative limit, rounds outside 1 .. 1024, unknown flags, null and misaligned pointers) returns before
// anything is launched, so the program needs no GPU -- which makes it the place for the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/geodesic_host_check.cpp nsdp_amd/csrc/geodesic.hip nsdp_amd/csrc/api.hip -o geodesic_host_check
//   ./geodesic_host_check
//
// The pointers it passes are small integers the entries must never dereference; a read of one would be the sanitizer's report.
// Exit status 0 and "ok" when every call came back as expected.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../include/nsdp_geodesic.h"
#include "../include/nsdp_hip.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s (last error: %s)\n", what, nsdp_last_error());
    ++failures;
  }
}

bool refused_with(int rc, const char *word, const char *entry) {
  return rc == NSDP_EINVAL && std::strstr(nsdp_last_error(), word) != nullptr && std::strstr(nsdp_last_error(), entry) != nullptr;
}

template <class T>
T *fake(uintptr_t v) { return reinterpret_cast<T *>(v); }

struct Lengths {
  const float *verts = fake<const float>(16);
  const int32_t *faces = fake<const int32_t>(16), *foff = fake<const int32_t>(16), *voff = fake<const int32_t>(16),
                *loff = fake<const int32_t>(16), *lent = fake<const int32_t>(16);
  int P = 2, B = 2, vcap = 8, fcap = 12;
  int32_t *nbr = fake<int32_t>(16);
  float *len = fake<float>(16);
  int call() const { return nsdp_mesh_edge_lengths(verts, P, faces, foff, voff, B, vcap, fcap, loff, lent, nbr, len, nullptr); }
};

struct Relax {
  const int32_t *loff = fake<const int32_t>(16), *nbr = fake<const int32_t>(16), *voff = fake<const int32_t>(16);
  const float *len = fake<const float>(16);
  int B = 2, vcap = 8, fcap = 12, P = 2, rounds = 3, flags = 0;
  float limit = 1.5f;
  float *dist = fake<float>(16);
  int32_t *changed = fake<int32_t>(16);
  int call() const { return nsdp_mesh_geodesic_relax(loff, nbr, len, voff, B, vcap, fcap, P, limit, rounds, flags, dist, changed, nullptr); }
};

}  // namespace

int main() {
  expect(nsdp_abi_version() >= 29, "ABI version 29");
  expect(nsdp_mesh_geodesic_block() == NSDP_GEODESIC_BLOCK, "the block size is the header's");
  expect(nsdp_mesh_edge_table_entries(0, 8, 12) == 0 && nsdp_mesh_edge_table_entries(65536, 8, 12) == 0 &&
             nsdp_mesh_edge_table_entries(2, 0, 12) == 0 && nsdp_mesh_edge_table_entries(2, 1048577, 12) == 0 &&
             nsdp_mesh_edge_table_entries(2, 8, 0) == 0 && nsdp_mesh_edge_table_entries(2, 8, 11184811) == 0,
         "size: refused sizes");
  expect(nsdp_mesh_edge_table_entries(2, 8, 12) == 72u && nsdp_mesh_edge_table_entries(1, 1048576, 11184810) == 67108860u,
         "size: 6 entries per face row");

  char what[160];
  const struct { int P, B, vcap, fcap; const char *word; } sizes[] = {
      {0, 2, 8, 12, "P=0"},         {65536, 2, 8, 12, "P=65536"},      {2, 0, 8, 12, "B=0"},          {2, -2, 8, 12, "B=-2"},
      {2, 65536, 8, 12, "B=65536"}, {2, 2, 0, 12, "vcap=0"},           {2, 2, -5, 12, "vcap=-5"},     {2, 2, 1048577, 12, "vcap=1048577"},
      {2, 2, 8, 0, "fcap=0"},       {2, 2, 8, -1, "fcap=-1"},          {2, 2, 8, 11184811, "fcap=11184811"}};
  for (const auto &row : sizes) {
    Lengths a;
    a.P = row.P, a.B = row.B, a.vcap = row.vcap, a.fcap = row.fcap;
    std::snprintf(what, sizeof what, "edge_lengths P=%d B=%d vcap=%d fcap=%d names '%s'", row.P, row.B, row.vcap, row.fcap, row.word);
    expect(refused_with(a.call(), row.word, "mesh_edge_lengths"), what);
    Relax r;
    r.P = row.P, r.B = row.B, r.vcap = row.vcap, r.fcap = row.fcap;
    r.limit = -1.f, r.rounds = 0, r.flags = 8, r.dist = nullptr;      // sizes are judged before values and pointers
    std::snprintf(what, sizeof what, "geodesic_relax P=%d B=%d vcap=%d fcap=%d names '%s'", row.P, row.B, row.vcap, row.fcap, row.word);
    expect(refused_with(r.call(), row.word, "mesh_geodesic_relax"), what);
  }
  {
    Relax r;      // values are judged before pointers
    r.dist = nullptr;
    r.limit = std::numeric_limits<float>::quiet_NaN();
    expect(refused_with(r.call(), "limit=", "mesh_geodesic_relax"), "a NaN limit");
    r.limit = -0.25f;
    expect(refused_with(r.call(), "limit=", "mesh_geodesic_relax"), "a negative limit");
    r.limit = -0.f;
    expect(refused_with(r.call(), "limit=", "mesh_geodesic_relax"), "a limit of -0");
    r.limit = -std::numeric_limits<float>::infinity();
    expect(refused_with(r.call(), "limit=", "mesh_geodesic_relax"), "a limit of -inf");
    r.limit = std::numeric_limits<float>::infinity();
    expect(refused_with(r.call(), "null", "mesh_geodesic_relax"), "+inf is a limit: the null pointer is named");
    r.limit = 0.f;
    expect(refused_with(r.call(), "null", "mesh_geodesic_relax"), "+0 is a limit: the null pointer is named");
    for (int rounds : {0, -1, 1025}) {
      Relax s;
      s.dist = nullptr, s.rounds = rounds;
      std::snprintf(what, sizeof what, "rounds=%d", rounds);
      expect(refused_with(s.call(), what, "mesh_geodesic_relax"), what);
    }
    for (int rounds : {1, 1024}) {
      Relax s;
      s.dist = nullptr, s.rounds = rounds;
      expect(refused_with(s.call(), "null", "mesh_geodesic_relax"), "rounds 1 and 1024 are taken: the null pointer is named");
    }
    for (int flags : {2, 3, -1, 1 << 30}) {
      Relax s;
      s.dist = nullptr, s.flags = flags;
      std::snprintf(what, sizeof what, "flags=%d", flags);
      expect(refused_with(s.call(), what, "mesh_geodesic_relax"), what);
    }
    Relax s;
    s.dist = nullptr, s.flags = NSDP_GEODESIC_NO_LOCAL;
    expect(refused_with(s.call(), "null", "mesh_geodesic_relax"), "NSDP_GEODESIC_NO_LOCAL is a flag: the null pointer is named");
  }
  for (int which = 0; which < 7; ++which) {
    Lengths a;
    if (which == 0) a.verts = nullptr;
    if (which == 1) a.faces = nullptr;
    if (which == 2) a.foff = nullptr;
    if (which == 3) a.voff = nullptr;
    if (which == 4) a.loff = nullptr;
    if (which == 5) a.lent = nullptr;
    if (which == 6) a.len = nullptr;
    expect(refused_with(a.call(), "null", "mesh_edge_lengths"), "edge_lengths: a null pointer");
  }
  for (int which = 0; which < 6; ++which) {
    Relax r;
    if (which == 0) r.loff = nullptr;
    if (which == 1) r.nbr = nullptr;
    if (which == 2) r.len = nullptr;
    if (which == 3) r.voff = nullptr;
    if (which == 4) r.dist = nullptr;
    if (which == 5) r.changed = nullptr;
    expect(refused_with(r.call(), "null", "mesh_geodesic_relax"), "geodesic_relax: a null pointer");
  }
  {
    Lengths a;      // pointers are judged before the alignment; nbr and len are read and written as pairs
    a.len = fake<float>(20);
    expect(refused_with(a.call(), "aligned", "mesh_edge_lengths"), "edge_lengths: len not 8-byte aligned");
    a.verts = nullptr;
    expect(refused_with(a.call(), "null", "mesh_edge_lengths"), "edge_lengths: a null pointer beside a misaligned one names the pointer");
    Lengths b;
    b.nbr = fake<int32_t>(12);
    expect(refused_with(b.call(), "aligned", "mesh_edge_lengths"), "edge_lengths: nbr not 8-byte aligned");
    Lengths c;
    c.verts = fake<const float>(18);
    expect(refused_with(c.call(), "aligned", "mesh_edge_lengths"), "edge_lengths: verts not 4-byte aligned");
    Relax r;
    r.nbr = fake<const int32_t>(20);
    expect(refused_with(r.call(), "aligned", "mesh_geodesic_relax"), "geodesic_relax: nbr not 8-byte aligned");
    r.changed = nullptr;
    expect(refused_with(r.call(), "null", "mesh_geodesic_relax"), "geodesic_relax: a null pointer beside a misaligned one names the pointer");
    Relax s;
    s.dist = fake<float>(18);
    expect(refused_with(s.call(), "aligned", "mesh_geodesic_relax"), "geodesic_relax: dist not 4-byte aligned");
    Relax t;
    t.changed = fake<int32_t>(17);
    expect(refused_with(t.call(), "aligned", "mesh_geodesic_relax"), "geodesic_relax: changed_out not 4-byte aligned");
  }
  if (failures) return 1;
  std::puts("ok");
  return 0;
}
