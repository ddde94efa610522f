"""Launch loop for timing the sampling head under tensor parallelism (run under rocprofv3 --kernel-trace --stats):
  * usdm_sample_final (contiguous [B][V] rows) against usdm_sample_final_seg (the same rows as nseg rank-major segments) at the
    7B's V = 42 003, B = 16, nseg = 8, top_k = 50 / top_p = 0.95 (every pass of the kernel runs);
  * usdm_logits_p2p, put and get halves (split form), 2 logical ranks on one GPU, at the 7B's Vloc for TP = 2 and TP = 8.
Single-GPU timing only: the logical ranks' exchange is local memory, not xGMI."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    from usdm_amd import ops
    from usdm_amd.llm import vocab_shard
    from usdm_amd.p2p import P2PComm
    dev = torch.device("cuda:0")
    V, B, nseg, Hd = 42003, 16, 8, 4096
    Vloc = vocab_shard(V, 0, nseg)[0]
    g = torch.Generator().manual_seed(0)
    rows = (torch.randn(B, V, generator=g) * 2).to(dev)
    seg = torch.zeros(nseg, B, Vloc, device=dev)
    for s in range(nseg):
        n = min(V, (s + 1) * Vloc) - s * Vloc
        seg[s, :, :n] = rows[:, s * Vloc:s * Vloc + n]
    E = torch.randn(V, Hd, generator=g).to(torch.bfloat16).to(dev)
    sp = ops.sample_params_tensor(dev, B).view(B, -1)
    for b in range(B):
        ops.set_sample_params(sp[b], 0.9, 50, 0.95, b)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    h = torch.zeros(B, Hd, dtype=torch.bfloat16, device=dev)
    st = ops.decode_state(i32(B), i32(B, 1 << 20), i32(B), i32(B), batch=B)   # max_out beyond the step count: no wrap
    for _ in range(a.iters):
        ops.sample_final(rows, st, dev_params=sp, embed=E, h_out=h, Hd=Hd)
        ops.sample_final(seg, st, dev_params=sp, V=V, nseg=nseg, seg_stride=B * Vloc, seg_len=Vloc, embed=E, h_out=h, Hd=Hd)
    torch.cuda.synchronize()
    for tp in (2, 8):
        vl = vocab_shard(V, 0, tp)[0]
        comms = P2PComm.in_process(2, 2 + -(-vl // Hd), Hd, timeout_ms=2000)
        loc = [torch.randn(vl, generator=g).to(dev) for _ in range(2)]
        out = [torch.zeros(2 * vl, device=dev) for _ in range(2)]
        for _ in range(a.iters):
            for r in range(2):
                ops.logits_p2p(loc[r], vl, None, comms[r], 2, out[r], phase=1)
            for r in range(2):
                ops.logits_p2p(loc[r], vl, None, comms[r], 2, out[r], phase=2)
        torch.cuda.synchronize()
        for c in comms:
            c.raise_if_failed()
        assert torch.equal(out[0], torch.cat(loc)) and torch.equal(out[1], out[0])
        print(f"logits exchange Vloc={vl}: ok, status {[c.status() for c in comms]}")
    print("done")


if __name__ == "__main__":
    main()
