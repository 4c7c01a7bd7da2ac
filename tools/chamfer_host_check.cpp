// The argument checks of include/nsdp_chamfer.h as a stand-alone host program: every refused call of the bad-argument table
// (refused sizes, weights that are not finite, null and misaligned pointers, lists that a non-zero weight needs) returns before
// anything is launched, so the program needs no GPU -- which makes it the place for the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/chamfer_host_check.cpp nsdp_amd/csrc/chamfer.hip nsdp_amd/csrc/eval_metric.hip nsdp_amd/csrc/api.hip -o chamfer_host_check
//   ./chamfer_host_check
//
// The pointers it passes are small integers the entries must never dereference; a read of one would be the sanitizer's report.
// Exit status 0 and "ok" when every call came back as expected.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/nsdp_chamfer.h"
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

struct ForwardArgs {
  const float *pred = fake<const float>(16), *target = fake<const float>(16);
  int B = 2, n = 5, m = 7;
  float w_pt = 1.f, w_tp = 1.f;
  void *ws = fake<void>(16);
  float *d_pt = fake<float>(16), *d_tp = fake<float>(16), *terms = fake<float>(16), *loss = fake<float>(16);
  int32_t *i_pt = fake<int32_t>(16), *i_tp = fake<int32_t>(16);
  int call() const { return nsdp_chamfer_forward(pred, target, B, n, m, w_pt, w_tp, ws, d_pt, i_pt, d_tp, i_tp, terms, loss, nullptr); }
};

struct BackwardArgs {
  const float *self = fake<const float>(16), *other = fake<const float>(16), *g = fake<const float>(16);
  const int32_t *idx = fake<const int32_t>(16), *offsets = fake<const int32_t>(16), *entries = fake<const int32_t>(16);
  int B = 2, n_self = 5, n_other = 7;
  float w_direct = 1.f, w_list = 1.f;
  float *grad = fake<float>(16);
  int call() const {
    return nsdp_chamfer_backward(self, other, idx, offsets, entries, g, B, n_self, n_other, w_direct, w_list, grad, nullptr);
  }
};

template <class Args>
void sizes(const char *name, int Args::*rows, int Args::*other_rows) {
  char what[96];
  const struct { int B, n, m; const char *word; } table[] = {
      {0, 5, 7, "batch"},        {-3, 5, 7, "batch"},     {65536, 5, 7, "batch"},           {2, 0, 7, "n=0"},
      {2, -1, 7, "n=-1"},        {2, 1048577, 7, "n=1048577"}, {2, 5, 0, "m=0"},            {2, 5, 1048577, "m=1048577"},
      {2048, 1048576, 7, "2^31"}, {65535, 7, 32769, "2^31"}};
  for (const auto &row : table) {
    Args a;
    a.B = row.B, a.*rows = row.n, a.*other_rows = row.m;
    std::snprintf(what, sizeof what, "%s: B=%d n=%d m=%d names '%s'", name, row.B, row.n, row.m, row.word);
    expect(refused_with(a.call(), row.word) && std::strstr(nsdp_last_error(), name) != nullptr, what);
  }
}

}  // namespace

int main() {
  expect(nsdp_abi_version() >= 18, "ABI version 18");
  // the size query: 0 for what the entry refuses, one double per shape otherwise
  expect(nsdp_chamfer_forward_workspace_bytes(0) == 0 && nsdp_chamfer_forward_workspace_bytes(-1) == 0 &&
             nsdp_chamfer_forward_workspace_bytes(65536) == 0, "size: refused B");
  expect(nsdp_chamfer_forward_workspace_bytes(1) == 8 && nsdp_chamfer_forward_workspace_bytes(65535) == 8u * 65535u, "size: 8 B");

  sizes<ForwardArgs>("chamfer_forward", &ForwardArgs::n, &ForwardArgs::m);
  sizes<BackwardArgs>("chamfer_backward", &BackwardArgs::n_self, &BackwardArgs::n_other);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  {
    ForwardArgs a;      // sizes are judged before pointers and weights
    a.pred = a.target = nullptr, a.ws = nullptr, a.d_pt = a.d_tp = a.terms = a.loss = nullptr, a.i_pt = a.i_tp = nullptr, a.n = 0, a.w_pt = nan;
    expect(refused_with(a.call(), "n=0"), "forward: a refused size beside null pointers names the size");
    ForwardArgs b, c, d;
    b.w_pt = nan, c.w_tp = inf, d.w_tp = -inf;
    expect(refused_with(b.call(), "finite") && refused_with(c.call(), "finite") && refused_with(d.call(), "finite"), "forward: weights");
  }
  for (int which = 0; which < 9; ++which) {
    ForwardArgs a;
    if (which == 0) a.pred = nullptr;
    if (which == 1) a.target = nullptr;
    if (which == 2) a.ws = nullptr;
    if (which == 3) a.d_pt = nullptr;
    if (which == 4) a.i_pt = nullptr;
    if (which == 5) a.d_tp = nullptr;
    if (which == 6) a.i_tp = nullptr;
    if (which == 7) a.terms = nullptr;
    if (which == 8) a.loss = nullptr;
    expect(refused_with(a.call(), "null"), "forward: a null pointer");
  }
  {
    ForwardArgs a;
    a.ws = fake<void>(20);
    expect(refused_with(a.call(), "aligned"), "forward: a workspace that is not 8-byte aligned");
  }

  {
    BackwardArgs a;
    a.self = a.other = a.g = nullptr, a.idx = a.offsets = a.entries = nullptr, a.grad = nullptr, a.n_other = 0;
    expect(refused_with(a.call(), "m=0"), "backward: a refused size beside null pointers names the size");
    BackwardArgs b, c;
    b.w_direct = nan, c.w_list = inf;
    expect(refused_with(b.call(), "finite") && refused_with(c.call(), "finite"), "backward: weights");
  }
  for (int which = 0; which < 5; ++which) {
    BackwardArgs a;
    if (which == 0) a.self = nullptr;
    if (which == 1) a.other = nullptr;
    if (which == 2) a.idx = nullptr;
    if (which == 3) a.g = nullptr;
    if (which == 4) a.grad = nullptr;
    expect(refused_with(a.call(), "null"), "backward: a null pointer");
  }
  {
    BackwardArgs a, b;      // lists go with a non-zero list weight
    a.offsets = nullptr;
    b.entries = nullptr;
    expect(refused_with(a.call(), "offsets") && refused_with(b.call(), "offsets"), "backward: a list weight without lists");
  }
  if (failures) return 1;
  std::puts("ok");
  return 0;
}
