// The argument checks of include/nsdp_handle_sets.h as a stand-alone host program: every refused call of the bad-argument table
// (refused sizes, both or neither of motions / targets, null and misaligned pointers) returns before anything is launched, so the
// program needs no GPU -- which makes it the place for the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/handle_sets_host_check.cpp nsdp_amd/csrc/handle_sets.hip nsdp_amd/csrc/api.hip -o handle_sets_host_check
//   ./handle_sets_host_check
//
// The pointers it passes are small integers the entries must never dereference; a read of one would be the sanitizer's report.
// Exit status 0 and "ok" when every call came back as expected.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/nsdp_handle_sets.h"
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

struct RowsArgs {
  const float *src = fake<const float>(16);
  const uint8_t *labels = fake<const uint8_t>(17);
  const float *motions = fake<const float>(16), *targets = nullptr;
  int B = 1, n = 8, H = 3, T = 1;
  float *rows = fake<float>(16), *tgt = fake<float>(16);
  uint8_t *ho = fake<uint8_t>(19);
  int call() const { return nsdp_handle_set_rows(src, labels, motions, targets, B, n, H, T, rows, tgt, ho, nullptr); }
};

struct PackedArgs {
  const float *src = fake<const float>(16);
  const int32_t *offsets = fake<const int32_t>(16);
  const uint8_t *labels = fake<const uint8_t>(17);
  const float *motions = fake<const float>(16), *targets = nullptr;
  int B = 1, cap = 8, H = 3;
  float *rows = fake<float>(16), *tgt = fake<float>(16);
  uint8_t *ho = fake<uint8_t>(19);
  int call() const { return nsdp_handle_set_rows_ragged(src, offsets, labels, motions, targets, B, cap, H, rows, tgt, ho, nullptr); }
};

template <class Args>
void both_or_neither_and_handles(const char *who) {
  char what[96];
  {
    Args a;
    a.targets = fake<const float>(16);
    std::snprintf(what, sizeof what, "%s: motions and targets", who);
    expect(refused_with(a.call(), "got both"), what);
    a.motions = nullptr, a.targets = nullptr;
    std::snprintf(what, sizeof what, "%s: neither motions nor targets", who);
    expect(refused_with(a.call(), "got neither"), what);
  }
  {
    Args a;
    a.H = 0;
    std::snprintf(what, sizeof what, "%s: H = 0 with motions", who);
    expect(refused_with(a.call(), "H=0"), what);
    a.H = 256;
    std::snprintf(what, sizeof what, "%s: H = 256", who);
    expect(refused_with(a.call(), "H=256"), what);
    a.H = -1;
    std::snprintf(what, sizeof what, "%s: H = -1", who);
    expect(refused_with(a.call(), "H=-1"), what);
    a.H = 0, a.motions = nullptr, a.targets = fake<const float>(18);      // (H is not read with targets: the next check speaks)
    std::snprintf(what, sizeof what, "%s: misaligned targets, H unread", who);
    expect(refused_with(a.call(), "aligned"), what);
  }
}

}  // namespace

int main() {
  expect(nsdp_abi_version() >= 17, "ABI version 17");

  {
    RowsArgs a;
    a.B = 0;
    expect(refused_with(a.call(), "batch 0"), "rows: B = 0");
    a.B = 65536;
    expect(refused_with(a.call(), "batch 65536"), "rows: B = 65536");
    a.B = 1, a.n = 0;
    expect(refused_with(a.call(), "n=0"), "rows: n = 0");
    a.n = (1 << 20) + 1;
    expect(refused_with(a.call(), "n=1048577"), "rows: n too large");
    a.n = 8, a.T = 0;
    expect(refused_with(a.call(), "T=0"), "rows: T = 0");
    a.T = -3;
    expect(refused_with(a.call(), "T=-3"), "rows: a negative T");
    a.T = 256, a.B = 256;
    expect(refused_with(a.call(), "T*B=65536"), "rows: T * B = 65536");
    a.T = 65535, a.B = 65535;
    expect(refused_with(a.call(), "T*B=4294836225"), "rows: T * B beyond 32 bits");
  }
  {
    RowsArgs a;      // sizes are judged before pointers
    a.src = nullptr, a.labels = nullptr, a.motions = nullptr, a.rows = a.tgt = nullptr, a.ho = nullptr, a.n = 0;
    expect(refused_with(a.call(), "n=0"), "rows: a refused size beside null pointers names the size");
  }
  both_or_neither_and_handles<RowsArgs>("rows");
  for (int which = 0; which < 5; ++which) {
    RowsArgs a, b;
    if (which == 0) a.src = nullptr, b.src = fake<const float>(18);
    if (which == 1) a.labels = nullptr;                                   // (bytes: any alignment)
    if (which == 2) a.rows = nullptr, b.rows = fake<float>(18);
    if (which == 3) b.motions = fake<const float>(18);
    if (which == 4) b.tgt = fake<float>(18);                              // (tgt is optional: null is legal, misaligned is not)
    if (which < 3) expect(refused_with(a.call(), "null"), "rows: a null pointer");
    if (which != 1) expect(refused_with(b.call(), "aligned"), "rows: a misaligned pointer");
  }

  {
    PackedArgs a;
    a.B = 0;
    expect(refused_with(a.call(), "batch 0"), "packed: B = 0");
    a.B = 65536;
    expect(refused_with(a.call(), "batch 65536"), "packed: B = 65536");
    a.B = 1, a.cap = 0;
    expect(refused_with(a.call(), "cap=0"), "packed: cap = 0");
    a.cap = -7;
    expect(refused_with(a.call(), "cap=-7"), "packed: a negative cap");
  }
  {
    PackedArgs a;      // sizes are judged before pointers
    a.src = nullptr, a.offsets = nullptr, a.labels = nullptr, a.motions = nullptr, a.rows = a.tgt = nullptr, a.ho = nullptr, a.cap = 0;
    expect(refused_with(a.call(), "cap=0"), "packed: a refused size beside null pointers names the size");
  }
  both_or_neither_and_handles<PackedArgs>("packed");
  for (int which = 0; which < 6; ++which) {
    PackedArgs a, b;
    if (which == 0) a.src = nullptr, b.src = fake<const float>(18);
    if (which == 1) a.offsets = nullptr, b.offsets = fake<const int32_t>(18);
    if (which == 2) a.labels = nullptr;
    if (which == 3) a.rows = nullptr, b.rows = fake<float>(18);
    if (which == 4) b.motions = fake<const float>(18);
    if (which == 5) b.tgt = fake<float>(18);
    if (which < 4) expect(refused_with(a.call(), "null"), "packed: a null pointer");
    if (which != 2) expect(refused_with(b.call(), "aligned"), "packed: a misaligned pointer");
  }
  if (failures) return 1;
  std::puts("ok");
  return 0;
}
