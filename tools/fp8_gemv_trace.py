"""Per-workgroup phase timeline of the decode GEMV shapes of the 7B, bf16 weights against quantization="fp8" weights (the same
matrix quantized), one launch each over cold weights: where the time of an fp8 launch goes (ramp, prologue, K loop).
Needs a library built with  USDM_EXTRA_HIPCC_FLAGS=-DUSDM_GEMV_TRACE python -m usdm_amd.build --force  (see tools/gemv_trace.py)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usdm_amd import _lib, ops  # noqa: E402
from usdm_amd.quant import Fp8Weight  # noqa: E402

dev = torch.device("cuda:0")
lib = _lib.lib
# (workgroup counts must not decrease from one shape to the next: trace rows of a larger earlier grid would stay behind)
for (name, N, K, act, norm, res) in (("o", 4096, 4096, 0, False, True), ("qkv", 6144, 4096, 0, True, False),
                                     ("down", 4096, 14336, 0, False, True), ("gate/up", 28672, 4096, 3, True, False)):
    for fmt in ("bf16", "fp8"):
        copies = max(3, int(1.2e9 // (N * K * (1 if fmt == "fp8" else 2))))
        Ws = []
        for _ in range(copies):
            W = (torch.randn(N, K, device=dev) * K ** -0.5).to(torch.bfloat16)
            Ws.append(Fp8Weight.from_matrix(W) if fmt == "fp8" else W)
            del W
        x = torch.randn(K, device=dev).to(torch.bfloat16)
        g = torch.ones(K, device=dev) if norm else None
        nout = N // 2 if act == 3 else N
        r = torch.randn(nout, device=dev).to(torch.bfloat16) if res else None
        y = torch.zeros(nout, device=dev, dtype=torch.bfloat16)
        for W in Ws:
            ops.gemv(W, x, N=N, K=K, norm_w=g, act=act, residual=r, y16=y)
        torch.cuda.synchronize()
        buf = np.zeros(8192 * 8, dtype=np.uint64)
        assert lib.usdm_dbg_gemv_trace(buf.ctypes.data_as(C.c_void_p), C.c_int(buf.size)) == 0
        t = buf.reshape(8192, 8)
        nwg = int((t[:, 0] != 0).sum())
        t = t[:nwg].astype(np.int64)
        t0 = t[:, 0].min()
        us = lambda a: a * 10 / 1e3
        span = us(t[:, 3].max() - t0)
        nbytes = N * K * (1 if fmt == "fp8" else 2) + (N if fmt == "fp8" else 0)
        print(f"{name} N{N} K{K} {fmt}: {nwg} workgroups, span to last K-loop end {span:.2f} us ({nbytes / span / 1e6:.2f} TB/s)")
        print("   start skew p50/p90/max      ", np.percentile(us(t[:, 0] - t0), [50, 90, 100]).round(2))
        print("   ring issue (entry->issued)  ", np.percentile(us(t[:, 1] - t[:, 0]), [50, 90]).round(2))
        print("   x staging (+norm) incl sync ", np.percentile(us(t[:, 2] - t[:, 1]), [50, 90]).round(2))
        print("   K loop + wave reduce        ", np.percentile(us(t[:, 3] - t[:, 2]), [10, 50, 90, 100]).round(2))
        print("   workgroup end (rel. kernel) ", np.percentile(us(t[:, 3] - t0), [10, 50, 90, 100]).round(2), flush=True)
        del Ws
