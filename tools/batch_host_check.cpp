// The argument checks of include/nsdp_batch.h as a stand-alone host program: every refused call of the bad-argument table of
// nsdp_subset_draw and nsdp_batch_assemble (refused sizes, unknown streams, values that are not finite, null and misaligned
// pointers) returns before anything is launched, so the program needs no GPU -- which makes it the place for the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/batch_host_check.cpp nsdp_amd/csrc/batch_assemble.hip nsdp_amd/csrc/api.hip -o batch_host_check
//   ./batch_host_check
//
// The pointers it passes are small integers the entries must never dereference; a read of one would be the sanitizer's report.
// Exit status 0 and "ok" when every call came back as expected.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/nsdp_batch.h"
#include "../include/nsdp_hip.h"

namespace {

int failures = 0, calls = 0;

void expect(bool ok, const char *what) {
  ++calls;
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s (last error: %s)\n", what, nsdp_last_error());
    ++failures;
  }
}

bool refused_with(int rc, const char *entry, const char *word) {
  return rc == NSDP_EINVAL && std::strstr(nsdp_last_error(), word) != nullptr && std::strstr(nsdp_last_error(), entry) != nullptr;
}

template <class T>
T *fake(uintptr_t v) { return reinterpret_cast<T *>(v); }

struct Draw {
  const int32_t *n_full = fake<const int32_t>(16);
  int B = 2, n_keep = 4, which = NSDP_DRAW_SURFACE;
  int32_t *rows = fake<int32_t>(16);
  int call() const { return nsdp_subset_draw(n_full, B, n_keep, 0x123456789ULL, 1u, 2u, which, rows, nullptr); }
};

struct Assemble {
  const void *surface = fake<const void>(16), *space = fake<const void>(32);
  long long surface_rows = 10, space_rows = 10;
  const int64_t *table = fake<const int64_t>(16);
  int n_frames = 2, B = 2, n = 4, m = 4;
  const int32_t *ids = fake<const int32_t>(16), *surf_idx = fake<const int32_t>(16), *space_idx = fake<const int32_t>(16);
  float partial_range = 0.1f, noise_level = 0.f;
  const float *noise = nullptr;
  float *surface_out = fake<float>(16), *inputs_out = fake<float>(16), *space_out = fake<float>(16);
  uint8_t *handle_out = fake<uint8_t>(17);
  int call() const {
    return nsdp_batch_assemble(surface, surface_rows, 1, space, space_rows, 0, table, n_frames, ids, B, surf_idx, n, space_idx, m,
                               partial_range, noise, noise_level, surface_out, handle_out, inputs_out, space_out, nullptr);
  }
};

}  // namespace

int main() {
  expect(nsdp_abi_version() >= 22, "ABI version 22");
  char what[160];
  {
    const struct { int B, n_keep, which; const char *word; } table[] = {
        {-1, 4, 0, "B=-1"},         {65536, 4, 0, "B=65536"},     {2, -3, 0, "n_keep=-3"}, {2, NSDP_BATCH_MAX_ROWS + 1, 0, "n_keep=1048577"},
        {4096, 1 << 20, 0, "too large"}, {2, 4, 2, "which=2"},    {2, 4, -1, "which=-1"}};
    for (const auto &row : table) {
      Draw d;
      d.B = row.B, d.n_keep = row.n_keep, d.which = row.which;
      std::snprintf(what, sizeof what, "subset_draw B=%d n_keep=%d which=%d names '%s'", row.B, row.n_keep, row.which, row.word);
      expect(refused_with(d.call(), "subset_draw", row.word), what);
    }
    Draw sizes_first;      // sizes are judged before pointers
    sizes_first.B = -1, sizes_first.n_full = nullptr, sizes_first.rows = nullptr;
    expect(refused_with(sizes_first.call(), "subset_draw", "B=-1"), "subset_draw: a refused size beside null pointers names the size");
    Draw a, b, c, d, e;
    a.n_full = nullptr, b.rows = nullptr, c.rows = fake<int32_t>(18), d.n_full = fake<const int32_t>(6);
    expect(refused_with(a.call(), "subset_draw", "null"), "subset_draw: null n_full");
    expect(refused_with(b.call(), "subset_draw", "null"), "subset_draw: null rows_out");
    expect(refused_with(c.call(), "subset_draw", "aligned"), "subset_draw: misaligned rows_out");
    expect(refused_with(d.call(), "subset_draw", "aligned"), "subset_draw: misaligned n_full");
    e.B = 0, e.n_full = nullptr, e.rows = nullptr;
    expect(e.call() == 0, "subset_draw: B = 0 is nothing to do");
    e.B = 2, e.n_keep = 0;
    expect(e.call() == 0, "subset_draw: n_keep = 0 is nothing to do");
  }
  {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const struct { int B, n, m, n_frames; long long surface_rows, space_rows; float partial_range, noise_level; const char *word; } table[] = {
        {-2, 4, 4, 2, 10, 10, 0.1f, 0.f, "B=-2"},
        {65536, 4, 4, 2, 10, 10, 0.1f, 0.f, "B=65536"},
        {2, -1, 4, 2, 10, 10, 0.1f, 0.f, "n=-1"},
        {2, 4, -1, 2, 10, 10, 0.1f, 0.f, "m=-1"},
        {2, NSDP_BATCH_MAX_ROWS + 1, 4, 2, 10, 10, 0.1f, 0.f, "n=1048577"},
        {2, 4, NSDP_BATCH_MAX_ROWS + 1, 2, 10, 10, 0.1f, 0.f, "m=1048577"},
        {1024, 1 << 17, 4, 2, 10, 10, 0.1f, 0.f, "too large"},
        {1024, 4, 1 << 17, 2, 10, 10, 0.1f, 0.f, "too large"},
        {2, 4, 4, 0, 10, 10, 0.1f, 0.f, "n_frames=0"},
        {2, 4, 4, -3, 10, 10, 0.1f, 0.f, "n_frames=-3"},
        {2, 4, 4, 2, 0, 10, 0.1f, 0.f, "surface_rows=0"},
        {2, 4, 4, 2, 10, -4, 0.1f, 0.f, "space_rows=-4"},
        {2, 4, 4, 2, 10, 10, nan, 0.f, "partial_range"},
        {2, 4, 4, 2, 10, 10, -inf, 0.f, "partial_range"},
        {2, 4, 4, 2, 10, 10, 0.1f, inf, "noise_level"},
        {2, 4, 4, 2, 10, 10, 0.1f, nan, "noise_level"}};
    for (const auto &row : table) {
      Assemble a;
      a.B = row.B, a.n = row.n, a.m = row.m, a.n_frames = row.n_frames, a.surface_rows = row.surface_rows, a.space_rows = row.space_rows;
      a.partial_range = row.partial_range, a.noise_level = row.noise_level;
      std::snprintf(what, sizeof what, "batch_assemble B=%d n=%d m=%d n_frames=%d rows=%lld/%lld names '%s'", row.B, row.n, row.m,
                    row.n_frames, row.surface_rows, row.space_rows, row.word);
      expect(refused_with(a.call(), "batch_assemble", row.word), what);
    }
    Assemble sizes_first;      // sizes are judged before pointers
    sizes_first.n_frames = 0, sizes_first.table = nullptr, sizes_first.ids = nullptr, sizes_first.surface = nullptr;
    expect(refused_with(sizes_first.call(), "batch_assemble", "n_frames=0"), "batch_assemble: a refused size beside null pointers names the size");
    for (int which = 0; which < 9; ++which) {
      Assemble a;
      if (which == 0) a.table = nullptr;
      if (which == 1) a.ids = nullptr;
      if (which == 2) a.surface = nullptr;
      if (which == 3) a.surf_idx = nullptr;
      if (which == 4) a.surface_out = nullptr;
      if (which == 5) a.handle_out = nullptr;
      if (which == 6) a.inputs_out = nullptr;
      if (which == 7) a.space = nullptr;
      if (which == 8) a.space_out = nullptr;
      expect(refused_with(a.call(), "batch_assemble", "null"), "batch_assemble: a null pointer");
    }
    Assemble a, b, c, d, e, f, g, h;
    a.surface = fake<const void>(24), b.space = fake<const void>(8), c.table = fake<const int64_t>(20), d.noise = fake<const float>(18);
    e.space_idx = fake<const int32_t>(6), f.surface_out = fake<float>(2);
    expect(refused_with(a.call(), "batch_assemble", "16-byte"), "batch_assemble: a surface arena that is not 16-byte aligned");
    expect(refused_with(b.call(), "batch_assemble", "16-byte"), "batch_assemble: a space arena that is not 16-byte aligned");
    expect(refused_with(c.call(), "batch_assemble", "8-byte"), "batch_assemble: a frame table that is not 8-byte aligned");
    expect(refused_with(d.call(), "batch_assemble", "4-byte"), "batch_assemble: misaligned noise");
    expect(refused_with(e.call(), "batch_assemble", "4-byte"), "batch_assemble: misaligned space_idx");
    expect(refused_with(f.call(), "batch_assemble", "4-byte"), "batch_assemble: misaligned surface_out");
    g.B = 0, g.table = nullptr, g.ids = nullptr;
    expect(g.call() == 0, "batch_assemble: B = 0 is nothing to do");
    h.n = 0, h.m = 0, h.table = nullptr, h.surface = nullptr, h.space = nullptr;
    expect(h.call() == 0, "batch_assemble: n = m = 0 is nothing to do");
    // a part without rows may come without its operands: the surviving refusal is the OTHER part's
    Assemble no_surface;
    no_surface.n = 0, no_surface.surface = nullptr, no_surface.surf_idx = nullptr, no_surface.surface_out = nullptr, no_surface.handle_out = nullptr;
    no_surface.inputs_out = nullptr, no_surface.surface_rows = 0, no_surface.space_out = nullptr;
    expect(refused_with(no_surface.call(), "batch_assemble", "space operands"), "batch_assemble: n = 0 leaves only the space operands to refuse");
  }
  if (failures) return 1;
  std::printf("ok: %d checks\n", calls);
  return 0;
}
