"""Per-workgroup phase timeline of the 7B's down_proj launch (bf16, N 4096, K 14336), the straight-line form (gemv_stream_kernel)
against gemv_kernel (usdm_gemv_args.resident = -1), one launch each over cold weights: when the first ring is issued, how long the
workgroup waits for x, and how long the 28 K iterations take.
Needs a library built with  USDM_EXTRA_HIPCC_FLAGS=-DUSDM_GEMV_TRACE python -m usdm_amd.build --force  (see tools/gemv_trace.py).
Stamps (100 MHz): 0 entry (skip word requested), 1 first ring issued, 2 x staged (behind the barrier), 3 K loop + wave reduce done."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usdm_amd import _lib, ops  # noqa: E402

dev = torch.device("cuda:0")
N, K = 4096, 14336
copies = 8       # 8 x 117 MB: a launch finds none of its weights in the 256 MB last-level cache
Ws = [(torch.randn(N, K, device=dev) * K ** -0.5).to(torch.bfloat16) for _ in range(copies)]
x = torch.randn(K, device=dev).to(torch.bfloat16)
h = torch.randn(N, device=dev).to(torch.bfloat16)
skip = torch.zeros(1, dtype=torch.int32, device=dev)
us = lambda a: a * 10 / 1e3
pct = lambda a, q: np.percentile(us(a), q).round(2)
for name, res in (("straight-line", 0), ("gemv_kernel", -1)):
    for rep in range(2):      # the second pass over the copies is the one reported (first: code and page tables cold)
        for W in Ws:
            ops.gemv(W, x, N=N, K=K, residual=h, y16=h, skip=skip, resident=res)
        torch.cuda.synchronize()
    buf = np.zeros(8192 * 8, dtype=np.uint64)
    assert _lib.lib.usdm_dbg_gemv_trace(buf.ctypes.data_as(C.c_void_p), C.c_int(buf.size)) == 0
    t = buf.reshape(8192, 8)[:N // 16].astype(np.int64)
    t0 = t[:, 0].min()
    span = us(t[:, 3].max() - t0)
    print(f"down_proj N{N} K{K} bf16, {name}: {t.shape[0]} workgroups, span to the last workgroup's end {span:.2f} us ({N * K * 2 / span / 1e6:.2f} TB/s)")
    print("   start skew p50/p90/max          ", pct(t[:, 0] - t0, [50, 90, 100]))
    print("   ring issue (entry->issued)      ", pct(t[:, 1] - t[:, 0], [50, 90]))
    print("   x wait + staging incl sync      ", pct(t[:, 2] - t[:, 1], [50, 90]))
    print("   K loop + wave reduce            ", pct(t[:, 3] - t[:, 2], [10, 50, 90, 100]))
    print("   workgroup end (rel. kernel)     ", pct(t[:, 3] - t0, [10, 50, 90, 100]), flush=True)
