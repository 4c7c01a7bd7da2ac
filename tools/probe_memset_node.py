"""Does a hipMemsetAsync captured as a node of a torch.cuda.graph take effect on every replay (graph.replay = hipGraphLaunch)?

    python tools/probe_memset_node.py

The captured chain: memset of the first 36 016 bytes of a buffer to 0 -> the sum of those bytes into `out` -> a fill of them
with 1 (dirty for the next replay).  With the memset in effect every replay leaves 0 in `out`.  Two buffers: one allocated
before the capture, one inside it.  Harmless: memsets and fills inside buffers of the process.  Prints the sums per replay and
MEMSET_OK / MEMSET_BROKEN; docs/EXPERIMENTS.md ("memset nodes") has what it printed on an MI355X."""
import ctypes
import sys

import torch

NB, SIZE, REPLAYS = 36016, 612624, 4


def run(hip, dev, inside):
    out = torch.zeros(1, dtype=torch.int64, device=dev)
    outer = torch.full((SIZE,), 1, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ws = torch.empty((SIZE,), dtype=torch.uint8, device=dev) if inside else outer
        rc = hip.hipMemsetAsync(ctypes.c_void_p(ws.data_ptr()), 0, NB, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
        out.copy_(ws[:NB].to(torch.int64).sum().reshape(1))      # reads what the memset left
        ws[:NB].fill_(1)                                         # dirty again for the next replay
        del ws
    res = []
    for _ in range(REPLAYS):
        g.replay()
        torch.cuda.synchronize()
        res.append(int(out))
    return res


def main():
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    hip.hipMemsetAsync.restype = ctypes.c_int
    dev = torch.device("cuda", 0)
    ok = True
    for inside in (False, True):
        r = run(hip, dev, inside)
        print("buffer allocated", "inside" if inside else "before", "the capture: sums behind the memset node per replay", r, flush=True)
        ok = ok and not any(r)
    print("MEMSET_OK" if ok else "MEMSET_BROKEN", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
