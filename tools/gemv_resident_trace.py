"""Per-workgroup phase timeline of the 7B's gate/up launch (bf16, N 28672, K 4096), resident form against one tile per workgroup,
one launch each over cold weights: how many prologues a CU pays and what happens between two tiles of a workgroup.
Needs a library built with  USDM_EXTRA_HIPCC_FLAGS=-DUSDM_GEMV_TRACE python -m usdm_amd.build --force  (see tools/gemv_trace.py).
Stamps (100 MHz): 0 entry, 1 first ring issued, 2 x staged and normalised, 3 K loop + wave reduce of the first tile done,
4 of the second tile (resident form only)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usdm_amd import _lib, ops  # noqa: E402

dev = torch.device("cuda:0")
N, K = 28672, 4096
copies = 6
Ws = [(torch.randn(N, K, device=dev) * K ** -0.5).to(torch.bfloat16) for _ in range(copies)]
x = torch.randn(K, device=dev).to(torch.bfloat16)
g = torch.ones(K, device=dev)
y = torch.zeros(N // 2, device=dev, dtype=torch.bfloat16)
us = lambda a: a * 10 / 1e3
pct = lambda a, q: np.percentile(us(a), q).round(2)
# (the resident form first: its grid is the smaller one, trace rows of a larger earlier grid would stay behind)
for name, res in (("resident", 0), ("one tile per workgroup", -1)):
    for rep in range(2):      # the second pass over the copies is the one reported (first: code and page tables cold)
        for W in Ws:
            ops.gemv(W, x, N=N, K=K, norm_w=g, act=3, y16=y, resident=res)
        torch.cuda.synchronize()
    buf = np.zeros(8192 * 8, dtype=np.uint64)
    assert _lib.lib.usdm_dbg_gemv_trace(buf.ctypes.data_as(C.c_void_p), C.c_int(buf.size)) == 0
    t = buf.reshape(8192, 8)
    nwg = int((t[:, 0] != 0).sum())
    t = t[:nwg].astype(np.int64)
    last = 4 if res == 0 and (t[:, 4] != 0).all() else 3
    t0 = t[:, 0].min()
    span = us(t[:, last].max() - t0)
    print(f"gate/up N{N} K{K} bf16, {name}: {nwg} workgroups, span to the last tile's end {span:.2f} us ({N * K * 2 / span / 1e6:.2f} TB/s)")
    print("   start skew p50/p90/max          ", pct(t[:, 0] - t0, [50, 90, 100]))
    print("   ring issue (entry->issued)      ", pct(t[:, 1] - t[:, 0], [50, 90]))
    print("   x staging + norm incl sync      ", pct(t[:, 2] - t[:, 1], [50, 90]))
    print("   first tile: K loop + wave reduce", pct(t[:, 3] - t[:, 2], [10, 50, 90, 100]))
    if last == 4:
        print("   second tile, from the first's end", pct(t[:, 4] - t[:, 3], [10, 50, 90, 100]))
    print("   workgroup end (rel. kernel)     ", pct(t[:, last] - t0, [10, 50, 90, 100]), flush=True)
