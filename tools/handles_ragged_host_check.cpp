// The argument checks of include/nsdp_handles_ragged.h as a stand-alone host program: every refused call of the bad-argument
// table (refused sizes, null and misaligned pointers, masks that do not go together) returns before anything is launched, so the
// program needs no GPU -- which makes it the place for the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/handles_ragged_host_check.cpp nsdp_amd/csrc/handles_ragged.hip nsdp_amd/csrc/api.hip -o handles_ragged_host_check
//   ./handles_ragged_host_check
//
// The pointers it passes are small integers the entries must never dereference; a read of one would be the sanitizer's report.
// Exit status 0 and "ok" when every call came back as expected.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/nsdp_handles_ragged.h"
#include "../include/nsdp_hip.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s (last error: %s)\n", what, nsdp_last_error());
    ++failures;
  }
}

bool refused_with(int rc, const char *word) { return rc == NSDP_EINVAL && std::strstr(nsdp_last_error(), word) != nullptr; }

template <class T>
T *fake(uintptr_t v) { return reinterpret_cast<T *>(v); }

struct BoundsArgs {
  const float *cano = fake<const float>(16);
  const int32_t *offsets = fake<const int32_t>(16);
  int B = 1, cap = 8, n_max = 8;
  void *ws = fake<void>(16);
  float *bounds = fake<float>(16);
  int call() const { return nsdp_handle_bounds_ragged(cano, offsets, B, cap, n_max, ws, bounds, nullptr); }
};

struct RowsArgs {
  const float *cano = fake<const float>(16), *src = fake<const float>(16);
  const int32_t *offsets = fake<const int32_t>(16);
  const float *bounds = fake<const float>(16);
  const uint32_t *params = fake<const uint32_t>(16);
  const uint8_t *hm = nullptr, *mm = nullptr;
  int B = 1, cap = 4;
  float *rows = fake<float>(16), *tgt = fake<float>(16);
  uint8_t *ho = fake<uint8_t>(16), *mo = fake<uint8_t>(17);
  int call() const { return nsdp_handle_rows_ragged(cano, src, offsets, bounds, params, hm, mm, B, cap, rows, tgt, ho, mo, nullptr); }
};

}  // namespace

int main() {
  expect(nsdp_abi_version() >= 16, "ABI version 16");
  // the size query: 0 for what the entry refuses, B * ceil(n_max / 4096) * 6 words otherwise
  expect(nsdp_handle_bounds_ragged_workspace_bytes(0, 8, 8) == 0 && nsdp_handle_bounds_ragged_workspace_bytes(65536, 8, 8) == 0, "size: B");
  expect(nsdp_handle_bounds_ragged_workspace_bytes(1, 0, 8) == 0 && nsdp_handle_bounds_ragged_workspace_bytes(1, -1, 8) == 0, "size: cap");
  expect(nsdp_handle_bounds_ragged_workspace_bytes(1, 8, 0) == 0 && nsdp_handle_bounds_ragged_workspace_bytes(1, 8, (1 << 20) + 1) == 0,
         "size: n_max");
  expect(nsdp_handle_bounds_ragged_workspace_bytes(3, 8, 4097) == 3u * 2u * 6u * 4u, "size: two partials per shape at 4097");
  expect(nsdp_handle_bounds_ragged_workspace_bytes(65535, 0x7fffffff, 1 << 20) == 65535ull * 256ull * 24ull, "size: the largest");

  {
    BoundsArgs a;
    a.B = 0;
    expect(refused_with(a.call(), "batch"), "bounds: B = 0");
    a.B = 65536;
    expect(refused_with(a.call(), "batch"), "bounds: B = 65536");
  }
  {
    BoundsArgs a;
    a.cap = 0;
    expect(refused_with(a.call(), "cap=0"), "bounds: cap = 0");
    a.cap = 8;
    a.n_max = 0;
    expect(refused_with(a.call(), "n_max=0"), "bounds: n_max = 0");
    a.n_max = (1 << 20) + 1;
    expect(refused_with(a.call(), "n_max=1048577"), "bounds: n_max too large");
  }
  {
    BoundsArgs a;      // sizes are judged before pointers
    a.cano = nullptr, a.offsets = nullptr, a.ws = nullptr, a.bounds = nullptr, a.n_max = 0;
    expect(refused_with(a.call(), "n_max=0"), "bounds: a refused size beside null pointers names the size");
  }
  for (int which = 0; which < 4; ++which) {
    BoundsArgs a, b;
    if (which == 0) a.cano = nullptr, b.cano = fake<const float>(18);
    if (which == 1) a.offsets = nullptr, b.offsets = fake<const int32_t>(18);
    if (which == 2) a.ws = nullptr, b.ws = fake<void>(18);
    if (which == 3) a.bounds = nullptr, b.bounds = fake<float>(18);
    expect(refused_with(a.call(), "null"), "bounds: a null pointer");
    expect(refused_with(b.call(), "aligned"), "bounds: a misaligned pointer");
  }

  {
    RowsArgs a;
    a.B = 0;
    expect(refused_with(a.call(), "batch"), "rows: B = 0");
    a.B = 65536;
    expect(refused_with(a.call(), "batch"), "rows: B = 65536");
    a.B = 1;
    a.cap = 0;
    expect(refused_with(a.call(), "cap=0"), "rows: cap = 0");
    a.cap = -7;
    expect(refused_with(a.call(), "cap=-7"), "rows: a negative cap");
  }
  {
    RowsArgs a;      // sizes are judged before pointers
    a.cano = a.src = a.bounds = nullptr, a.offsets = nullptr, a.params = nullptr, a.rows = a.tgt = nullptr, a.ho = a.mo = nullptr, a.cap = 0;
    expect(refused_with(a.call(), "cap=0"), "rows: a refused size beside null pointers names the size");
  }
  {
    RowsArgs a;
    a.hm = fake<const uint8_t>(16);
    expect(refused_with(a.call(), "go together"), "rows: handle_mask alone");
    a.hm = nullptr, a.mm = fake<const uint8_t>(16);
    expect(refused_with(a.call(), "go together"), "rows: move_mask alone");
  }
  for (int which = 0; which < 7; ++which) {
    RowsArgs a, b;
    if (which == 0) a.cano = nullptr, b.cano = fake<const float>(18);
    if (which == 1) a.src = nullptr, b.src = fake<const float>(18);
    if (which == 2) a.offsets = nullptr, b.offsets = fake<const int32_t>(18);
    if (which == 3) a.bounds = nullptr, b.bounds = fake<const float>(18);
    if (which == 4) a.params = nullptr, b.params = fake<const uint32_t>(18);
    if (which == 5) a.rows = nullptr, b.rows = fake<float>(18);
    if (which == 6) b.tgt = fake<float>(18);      // (tgt is optional: null is legal, misaligned is not)
    if (which != 6) expect(refused_with(a.call(), "null"), "rows: a null pointer");
    expect(refused_with(b.call(), "aligned"), "rows: a misaligned pointer");
  }
  {
    RowsArgs a;      // the mask form does not need cano and bounds -- but still needs src, and alignment
    a.hm = fake<const uint8_t>(17), a.mm = fake<const uint8_t>(19), a.cano = nullptr, a.bounds = nullptr, a.src = nullptr;
    expect(refused_with(a.call(), "null"), "rows: the mask form without src");
    a.src = fake<const float>(16), a.rows = fake<float>(18);
    expect(refused_with(a.call(), "aligned"), "rows: the mask form with misaligned rows");
  }
  if (failures) return 1;
  std::puts("ok");
  return 0;
}
