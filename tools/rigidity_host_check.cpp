// The argument checks of include/nsdp_rigidity.h as a stand-alone host program: every refused call of the bad-argument table
// (refused sizes, a weight that is not finite, null and misaligned pointers) returns before anything is launched, so the program
// needs no GPU -- which makes it the place for the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/rigidity_host_check.cpp nsdp_amd/csrc/rigidity.hip nsdp_amd/csrc/api.hip -o rigidity_host_check
//   ./rigidity_host_check
//
// The pointers it passes are small integers the entries must never dereference; a read of one would be the sanitizer's report.
// Exit status 0 and "ok" when every call came back as expected.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/nsdp_hip.h"
#include "../include/nsdp_rigidity.h"

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
  const float *pred = fake<const float>(16), *source = fake<const float>(16);
  const int32_t *idx = fake<const int32_t>(16);
  int B = 2, n = 5, K = 3;
  float w = 1.f;
  void *ws = fake<void>(16);
  float *resid = fake<float>(16), *terms = fake<float>(16), *loss = fake<float>(16);
  int call() const { return nsdp_rigidity_forward(pred, source, idx, B, n, K, w, ws, resid, terms, loss, nullptr); }
};

struct BackwardArgs {
  const float *pred = fake<const float>(16), *resid = fake<const float>(16), *g = fake<const float>(16);
  const int32_t *idx = fake<const int32_t>(16), *offsets = fake<const int32_t>(16), *entries = fake<const int32_t>(16);
  int B = 2, n = 5, K = 3;
  float w = 1.f;
  float *grad = fake<float>(16);
  int call() const { return nsdp_rigidity_backward(pred, idx, resid, offsets, entries, g, B, n, K, w, grad, nullptr); }
};

template <class Args>
void sizes(const char *name) {
  char what[96];
  const struct { int B, n, K; const char *word; } table[] = {
      {0, 5, 3, "batch"},     {-3, 5, 3, "batch"},          {65536, 5, 3, "batch"},        {2, 0, 3, "n=0"},
      {2, -1, 3, "n=-1"},     {2, 1048577, 3, "n=1048577"}, {2, 5, 0, "K=0"},              {2, 5, -2, "K=-2"},
      {2, 5, 33, "K=33"},     {64, 1048576, 32, "2^31"},    {65535, 32769, 1, "2^31"},     {2048, 1048576, 1, "2^31"}};
  for (const auto &row : table) {
    Args a;
    a.B = row.B, a.n = row.n, a.K = row.K;
    std::snprintf(what, sizeof what, "%s: B=%d n=%d K=%d names '%s'", name, row.B, row.n, row.K, row.word);
    expect(refused_with(a.call(), row.word) && std::strstr(nsdp_last_error(), name) != nullptr, what);
  }
}

}  // namespace

int main() {
  expect(nsdp_abi_version() >= 20, "ABI version 20");
  // the size query: 0 for what the entry refuses, 65 doubles per shape otherwise
  expect(nsdp_rigidity_forward_workspace_bytes(0) == 0 && nsdp_rigidity_forward_workspace_bytes(-1) == 0 &&
             nsdp_rigidity_forward_workspace_bytes(65536) == 0, "size: refused B");
  expect(nsdp_rigidity_forward_workspace_bytes(1) == 520 && nsdp_rigidity_forward_workspace_bytes(65535) == 520u * 65535u, "size: 520 B");

  sizes<ForwardArgs>("rigidity_forward");
  sizes<BackwardArgs>("rigidity_backward");
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  {
    ForwardArgs a;      // sizes are judged before pointers and the weight
    a.pred = a.source = nullptr, a.idx = nullptr, a.ws = nullptr, a.resid = a.terms = a.loss = nullptr, a.n = 0, a.w = nan;
    expect(refused_with(a.call(), "n=0"), "forward: a refused size beside null pointers names the size");
    ForwardArgs b, c, d, e;
    b.w = nan, c.w = inf, d.w = -inf;
    expect(refused_with(b.call(), "finite") && refused_with(c.call(), "finite") && refused_with(d.call(), "finite"), "forward: weight");
    e.B = 1, e.n = 1048576, e.K = 32, e.pred = nullptr;      // (the largest shape is a size the entry takes: the pointer is named)
    expect(refused_with(e.call(), "null"), "forward: the largest shape beside a null pointer names the pointer");
  }
  for (int which = 0; which < 7; ++which) {
    ForwardArgs a;
    if (which == 0) a.pred = nullptr;
    if (which == 1) a.source = nullptr;
    if (which == 2) a.idx = nullptr;
    if (which == 3) a.ws = nullptr;
    if (which == 4) a.resid = nullptr;
    if (which == 5) a.terms = nullptr;
    if (which == 6) a.loss = nullptr;
    expect(refused_with(a.call(), "null"), "forward: a null pointer");
  }
  {
    ForwardArgs a;
    a.ws = fake<void>(20);
    expect(refused_with(a.call(), "aligned"), "forward: a workspace that is not 8-byte aligned");
  }

  {
    BackwardArgs a;
    a.pred = a.resid = a.g = nullptr, a.idx = a.offsets = a.entries = nullptr, a.grad = nullptr, a.K = 0;
    expect(refused_with(a.call(), "K=0"), "backward: a refused size beside null pointers names the size");
    BackwardArgs b, c;
    b.w = nan, c.w = inf;
    expect(refused_with(b.call(), "finite") && refused_with(c.call(), "finite"), "backward: weight");
  }
  for (int which = 0; which < 7; ++which) {
    BackwardArgs a;
    if (which == 0) a.pred = nullptr;
    if (which == 1) a.idx = nullptr;
    if (which == 2) a.resid = nullptr;
    if (which == 3) a.offsets = nullptr;
    if (which == 4) a.entries = nullptr;
    if (which == 5) a.g = nullptr;
    if (which == 6) a.grad = nullptr;
    expect(refused_with(a.call(), "null"), "backward: a null pointer");
  }
  if (failures) return 1;
  std::puts("ok");
  return 0;
}
