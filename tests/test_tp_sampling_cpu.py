"""CPU: the host side of sampling under tensor parallelism.
  * seed agreement: ranks whose torch generators differ all sample with rank 0's seed (usdm_amd.llm.agree_seed over a world-size-2
    gloo group, the transport the single-GPU multi-rank validation uses);
  * site sizing of the peer-to-peer logits exchange (P2PComm.sites_needed) at the 7B's vocabulary;
  * argument checks of the two new entry points (usdm_sample_final_seg, usdm_logits_p2p): refused with a message, never launched."""
import ctypes
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from usdm_amd.llm import agree_seed
    torch.manual_seed(100 + 17 * rank)                    # a different generator state on every rank
    drawn = int(torch.randint(0, 2 ** 62, (1,)).item())    # what generate() draws for seed=None
    got = agree_seed(drawn, dist.group.WORLD, rank)
    explicit = agree_seed(2 ** 62 + 12345, dist.group.WORLD, rank)   # every rank passes the same explicit seed
    out_q.put((rank, drawn, got, explicit))
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_seed_agreement_over_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=150) for _ in range(2))
    for p in procs:
        p.join(30)
    (_, d0, g0, e0), (_, d1, g1, e1) = res
    assert d0 != d1, "the ranks' own draws should differ (different generator states)"
    assert g0 == g1 == d0, "every rank must sample with rank 0's seed"
    assert e0 == e1 == 2 ** 62 + 12345


def test_sites_needed_7b_vocab():
    from usdm_amd.p2p import P2PComm
    cfg = dict(vocab_size=42003, hidden_size=4096, num_hidden_layers=32)
    # Vloc = ceil(42003 / tp): 21002 -> 6 sites of 4096, 10501 -> 3, 5251 -> 2
    assert [P2PComm.sites_needed(cfg, tp, True) for tp in (2, 4, 8)] == [65 + 6, 65 + 3, 65 + 2]
    assert [P2PComm.sites_needed(cfg, tp, False) for tp in (2, 4, 8)] == [65, 65, 65]     # greedy: 2L + 1, as before
    assert P2PComm.sites_needed(cfg, 8, True, max_elems=8192) == 66


def test_new_entry_points_refuse_bad_arguments():
    from usdm_amd import _lib
    lib = _lib.lib
    i32 = (ctypes.c_int32 * 4)()
    out = (ctypes.c_int32 * 4)()
    st = _lib.DecodeState()
    p = ctypes.cast(i32, ctypes.c_void_p)
    st.next_token, st.out_tokens, st.step, st.pos, st.max_out = p, ctypes.cast(out, ctypes.c_void_p), p, p, 4
    a = _lib.SampleArgs()
    a.logits, a.V, a.temperature, a.top_k, a.top_p = p, 1000, 1.0, 0, 1.0
    # segments that do not cover V
    rc = lib.usdm_sample_final_seg(ctypes.byref(a), ctypes.c_int32(2), ctypes.c_int64(600), ctypes.c_int32(400), ctypes.byref(st),
                                   None, ctypes.c_int32(0), None, None)
    assert rc == 2 and b"cover V" in lib.usdm_last_error()
    # overlapping segments
    rc = lib.usdm_sample_final_seg(ctypes.byref(a), ctypes.c_int32(2), ctypes.c_int64(100), ctypes.c_int32(500), ctypes.byref(st),
                                   None, ctypes.c_int32(0), None, None)
    assert rc == 2 and b"overlap" in lib.usdm_last_error()
    # seg_len 1 is outside the kernel's index arithmetic
    a.V = 4
    rc = lib.usdm_sample_final_seg(ctypes.byref(a), ctypes.c_int32(4), ctypes.c_int64(1), ctypes.c_int32(1), ctypes.byref(st),
                                   None, ctypes.c_int32(0), None, None)
    assert rc == 2
    # logits exchange: phase outside 0..2, missing output row
    rc = lib.usdm_logits_p2p(p, ctypes.c_int32(10), ctypes.byref(st), p, ctypes.c_int32(0), ctypes.c_int32(3), p, None)
    assert rc == 2 and b"usdm_logits_p2p" in lib.usdm_last_error()
    rc = lib.usdm_logits_p2p(p, ctypes.c_int32(10), ctypes.byref(st), p, ctypes.c_int32(0), ctypes.c_int32(2), None, None)
    assert rc == 2


def test_sample_final_refuses_cpu_tensors_on_the_segmented_form():
    from usdm_amd import _lib, ops
    st = ops.decode_state(torch.zeros(1, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                          torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.UsdmError):
        ops.sample_final(torch.zeros(2, 1, 8), st, V=15, nseg=2, seg_stride=8, seg_len=8)


def test_sample_final_refuses_a_segmented_tensor_without_seg_len(monkeypatch):
    """A [nseg][B][seg_len] tensor on the contiguous form would be read with a wrong row stride: refused before any launch."""
    from usdm_amd import ops
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)      # reach the shape check on the CPU
    st = ops.decode_state(torch.zeros(2, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                          torch.zeros(2, dtype=torch.int32), batch=2)
    with pytest.raises(ValueError, match="seg_len"):
        ops.sample_final(torch.zeros(1, 2, 8), st)
