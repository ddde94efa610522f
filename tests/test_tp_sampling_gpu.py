"""Sampling under tensor parallelism, validated on one MI355X:
  1. usdm_sample_final_seg (the sampler over a row of rank-major segments) against usdm_sample_final on the same logical rows;
  2. the single-sequence collective form: at every step (the prefill's pick included) the token equals the sampling oracle on the
     gathered row, on 2 logical ranks in lockstep and on a 1-rank RCCL group; seeds left to the model agree across ranks, and a
     sampled EOS stops every rank at the same step;
  3. serving.LLM on 2 logical ranks: sampled requests ride the continuous batch and equal the same request served alone;
  4. the peer-to-peer form (usdm_logits_p2p): split (lockstep) and fused (two streams) forms give the collective form's tokens,
     one epoch per token, and a communicator without the logits sites refuses sampling with the count it needs.
What one GPU cannot show is xGMI visibility and timing."""
import os
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = dict(vocab_size=1003, hidden_size=512, intermediate_size=1024, num_hidden_layers=3, num_attention_heads=8,
           num_key_value_heads=4, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)
BAD = [[i] for i in range(100, 400)]
SETTINGS = [(1.0, 0, 1.0), (0.8, 50, 0.95), (1.3, 0, 0.9)]     # (temperature, top_k, top_p)


def _sd():
    from oracle import mistral_oracle as MO
    return MO.random_state_dict(CFG, seed=13)


def _ids(dev, n=21, seed=4):
    return torch.randint(0, 1000, (1, n), generator=torch.Generator().manual_seed(seed)).to(dev)


# ---------------------------------------------------------------------------------------------------------------- 1. kernel
def _rows(B, V, Vloc, g):
    """B logical rows with the hard cases in the first four slots; knobs per slot."""
    rows = (torch.randn(B, V, generator=g) * 2).to(torch.bfloat16).float()
    knobs = []
    for b in range(B):
        kind = b % 5
        if kind == 0:
            knobs.append((1.0, 1, 1.0))                       # greedy slot
        elif kind == 1:
            knobs.append((1.0, 0, 0.9))                       # top-p only (the demo's default state)
        elif kind == 2:                                       # top_k = 200, k-th value tied across a segment boundary
            t = Vloc if Vloc < V else V // 2                  # first id of segment 1 (one segment: any interior id)
            ids = torch.randperm(V, generator=g)[:400]
            ids = ids[(ids != t - 1) & (ids != t)][:199]
            rows[b, ids] = 10.0 + torch.arange(199, dtype=torch.float32) / 64
            rows[b, t - 1] = rows[b, t] = 9.5
            knobs.append((0.9, 200, 1.0))
        elif kind == 3:
            rows[b] = float("-inf")                           # all banned: fallback pick
            knobs.append((1.0, 0, 1.0))
        else:
            knobs.append((0.7 + 0.1 * b, 40 * b, 0.97))
    return rows, knobs


@pytest.mark.parametrize("nseg", [1, 2, 8])
@pytest.mark.parametrize("B", [1, 6, 16])
def test_sample_final_seg_matches_contiguous(dev, nseg, B):
    from oracle import sampling_oracle as so
    from usdm_amd import ops
    from usdm_amd.llm import vocab_shard
    V, Hd = 42003, 64
    Vloc = vocab_shard(V, 0, nseg)[0]
    g = torch.Generator().manual_seed(100 * nseg + B)
    rows, knobs = _rows(B, V, Vloc, g)
    seg = torch.randn(nseg, B, Vloc, generator=g) * 1e3       # finite junk everywhere, the last segment's padding slots included
    for s in range(nseg):
        n = min(V, (s + 1) * Vloc) - s * Vloc
        seg[s, :, :n] = rows[:, s * Vloc:s * Vloc + n]
    rows, seg = rows.to(dev), seg.to(dev)
    E = torch.randn(V, Hd, generator=g).to(torch.bfloat16).to(dev)
    sp = ops.sample_params_tensor(dev, B).view(B, -1)
    for b, (T, k, p) in enumerate(knobs):
        ops.set_sample_params(sp[b], T, k, p, 1000 + b)
    steps0 = torch.arange(B, dtype=torch.int32) * 3 + 1

    def run(seg_form):
        nxt, stp = torch.zeros(B, dtype=torch.int32, device=dev), steps0.clone().to(dev)
        pos = torch.full((B,), 7, dtype=torch.int32, device=dev)
        out = torch.zeros(B, 64, dtype=torch.int32, device=dev)
        h = torch.zeros(B, Hd, dtype=torch.bfloat16, device=dev)
        probs = torch.full((B, V), -1.0, device=dev)
        if B == 1:
            st = ops.decode_state(nxt, out[0], stp, pos)
        else:
            st = ops.decode_state(nxt, out, stp, pos, batch=B)
        dp = sp[0] if B == 1 else sp
        if seg_form:
            ops.sample_final(seg, st, dev_params=dp, V=V, nseg=nseg, seg_stride=B * Vloc, seg_len=Vloc, probs_out=probs, embed=E,
                             h_out=h, Hd=Hd)
        else:
            ops.sample_final(rows[0] if B == 1 else rows, st, dev_params=dp, probs_out=probs, embed=E, h_out=h, Hd=Hd)
        torch.cuda.synchronize()
        return nxt, out, stp, pos, h, probs
    a, b_ = run(False), run(True)
    for x, y in zip(a, b_):
        assert torch.equal(x, y)
    if B > 3:
        assert int(a[0][3].item()) == 0           # all banned, nothing finite: id 0
    if nseg == 8 and B == 6:      # one configuration against the oracle (same seed, same step)
        for b in range(B):
            if b % 5 == 3:
                continue
            T, k, p = knobs[b]
            tok, _ = so.sample(rows[b].cpu().numpy(), int(steps0[b]), T, k, p, 1000 + b)
            assert int(b_[0][b].item()) == tok, b


# ------------------------------------------------------------------------------------- lockstep driver of the sampled step
def _run_lockstep(seg_lists):
    from usdm_amd import ops
    n = len(seg_lists[0])
    assert all(len(s) == n for s in seg_lists)
    for k in range(n):
        for segs in seg_lists:
            s = segs[k]
            if isinstance(s, ops.Plan):
                s.run()
            else:
                s()


@torch.no_grad()
def lockstep_sample(models, ids, new, T, k, p, seed, oracle=False):
    """Sampled generation with every logical rank stepping together; with oracle=True every step's token (the prefill's pick
    included) is checked against the sampling oracle on the gathered row rank 0 holds.  Returns rank 0's tokens."""
    from oracle import sampling_oracle as so
    from usdm_amd import ops
    V = CFG["vocab_size"]
    for m in models:
        ops.set_sample_params(m.sample_params, T, k, p, seed)
    _run_lockstep([m._setup_call(ids, 0, True, BAD, None, 0)[0] for m in models])

    def check(step):
        if oracle:
            torch.cuda.synchronize()
            tok, _ = so.sample(models[0].last_logits[:V].cpu().numpy(), step, T, k, p, seed)
            assert int(models[0].st_out[step].item()) == tok, f"step {step}"
    check(0)
    decode = [m._build_decode(True) for m in models]
    for s in range(1, new):
        _run_lockstep(decode)
        check(s)
    torch.cuda.synchronize()
    outs = [m.st_out[:new].tolist() for m in models]
    for m in models:
        assert int(m.st_step.item()) == new
        if m.p2p is not None:
            m.p2p.raise_if_failed()
    assert all(o == outs[0] for o in outs), "logical ranks disagree on the sampled tokens"
    assert all(t not in range(100, 400) for t in outs[0])
    return outs[0]


def _ranks(dev, tp, grp, comms=None, **kw):
    from usdm_amd.llm import USDMForCausalLM
    sd = _sd()
    return [USDMForCausalLM.from_state_dict(sd, CFG, dev, ctx_max=128, tp_rank=r, tp_size=tp, group=grp,
                                            p2p=comms[r] if comms else None, **kw) for r in range(tp)]


def _threaded(fns, grp=None, timeout=120):
    outs, errs = [None] * len(fns), [None] * len(fns)
    grp_abort = [grp._bar.abort] if grp is not None else []

    def work(r):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                outs[r] = fns[r]()
                torch.cuda.current_stream().synchronize()
        except Exception as e:  # noqa: BLE001 - reported below
            errs[r] = e
            for a in grp_abort:
                try:
                    a()
                except Exception:  # noqa: BLE001
                    pass
    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(len(fns))]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout)
    assert not any(t.is_alive() for t in th), "a rank is stuck"
    assert errs == [None] * len(fns), errs
    return outs


# --------------------------------------------------------------------------------------- 2. single sequence, collective form
def test_single_sequence_two_logical_ranks_vs_oracle(dev):
    from usdm_amd.p2p import InProcessGroup
    ranks = _ranks(dev, 2, InProcessGroup(2))
    ids = _ids(dev)
    for i, (T, k, p) in enumerate(SETTINGS):
        lockstep_sample(ranks, ids, 10, T, k, p, 77 + i, oracle=True)


def test_single_sequence_single_rank_rccl_vs_oracle(dev):
    import torch.distributed as dist
    from oracle import sampling_oracle as so
    from usdm_amd.llm import USDMForCausalLM
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29547")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        created = True
    try:
        m = USDMForCausalLM.from_state_dict(_sd(), CFG, dev, ctx_max=128, tp_segments=True, group=dist.group.WORLD)
        ids = _ids(dev)
        for i, (T, k, p) in enumerate(SETTINGS):
            ref = lockstep_sample([m], ids, 10, T, k, p, 91 + i, oracle=True)
            # generate() on the same model (captured graph): the same stream for the same explicit seed
            out = m.generate(input_ids=ids, max_new_tokens=10, do_sample=True, temperature=T, top_k=k or None, top_p=p, seed=91 + i,
                             bad_words_ids=BAD)[0, ids.shape[1]:].tolist()
            assert out == ref
            torch.manual_seed(5)
            a = m.generate(input_ids=ids, max_new_tokens=6, do_sample=True, temperature=T, bad_words_ids=BAD)
            assert a.shape[1] == ids.shape[1] + 6
            V = CFG["vocab_size"]
            assert so.sample(m.last_logits[:V].cpu().numpy(), 5, T, 0, 1.0, int(m.sample_params.view(torch.int64)[2].item()))[0] \
                == int(a[0, -1].item())
    finally:
        if created:
            dist.destroy_process_group()


def test_seed_agreement_and_eos_two_threaded_ranks(dev):
    from usdm_amd.p2p import InProcessGroup
    grp = InProcessGroup(2, threaded=True)
    ranks = _ranks(dev, 2, grp)
    ids = _ids(dev)
    os.environ["USDM_NO_GRAPH"] = "1"          # two threads capturing at once would trip over each other; launches stay eager
    try:
        # seed=None: every rank draws from torch's global generator, one after the other -> different draws; rank 0's is used
        torch.manual_seed(3)
        outs = _threaded([lambda r=r: ranks[r].generate(input_ids=ids, max_new_tokens=12, do_sample=True, temperature=1.2,
                                                         bad_words_ids=BAD)[0].tolist() for r in range(2)], grp)
        assert outs[0] == outs[1]
        seeds = [int(m.sample_params.view(torch.int64)[2].item()) for m in ranks]
        assert seeds[0] == seeds[1]
        # a sampled EOS stops every rank at the same step
        full = _threaded([lambda r=r: ranks[r].generate(input_ids=ids, max_new_tokens=12, do_sample=True, temperature=1.2, seed=5,
                                                         bad_words_ids=BAD)[0, ids.shape[1]:].tolist() for r in range(2)], grp)
        assert full[0] == full[1]
        eos = full[0][4]
        j = full[0].index(eos)
        cut = _threaded([lambda r=r: ranks[r].generate(input_ids=ids, max_new_tokens=12, do_sample=True, temperature=1.2, seed=5,
                                                        bad_words_ids=BAD, eos_token_id=eos)[0, ids.shape[1]:].tolist() for r in range(2)], grp)
        assert cut[0] == cut[1] == full[0][:j + 1]
        assert [int(m.st_step.item()) for m in ranks] == [j + 1, j + 1]
        # Python logits processors stay refused under tensor parallelism, with their own message
        with pytest.raises(NotImplementedError, match="logits processors under tensor parallelism"):
            ranks[0]._build_decode("hook")
    finally:
        os.environ.pop("USDM_NO_GRAPH", None)


# ------------------------------------------------------------------------------------------------------- 3. serving under TP
def _requests():
    from usdm_amd.serving import SamplingParams
    g = torch.Generator().manual_seed(9)
    prompts = [torch.randint(0, 1000, (19 + 3 * i,), generator=g).tolist() for i in range(6)]
    sps = []
    for i in range(6):
        if i % 2 == 0:
            sps.append(SamplingParams(temperature=0.0, max_tokens=10 + i))
        else:
            sps.append(SamplingParams(temperature=0.9, top_k=[-1, 40, -1][i // 2], top_p=[0.9, 1.0, 0.95][i // 2], seed=300 + i,
                                      max_tokens=9 + i))
    return prompts, sps


def test_serving_two_logical_ranks_batches_sampled_requests(dev):
    from usdm_amd import serving
    from usdm_amd.p2p import InProcessGroup
    grp = InProcessGroup(2, threaded=True)
    ranks = _ranks(dev, 2, grp)
    prompts, sps = _requests()
    ban = lambda hist, lg: torch.where((torch.arange(lg.numel(), device=lg.device) >= 100) & (torch.arange(lg.numel(), device=lg.device) < 400),
                                       torch.full_like(lg, float("-inf")), lg)
    for sp in sps:
        sp.logits_processors = [ban]
    greedy_ix = [i for i in range(6) if sps[i].temperature == 0.0]
    samp_ix = [i for i in range(6) if i not in greedy_ix]
    os.environ["USDM_NO_GRAPH"] = "1"
    try:
        def serve(r, slots):
            llm = serving.LLM(model=ranks[r], max_num_seqs=slots)
            mixed = [o.outputs[0].token_ids for o in llm.generate(prompt_token_ids=prompts, sampling_params=sps)]
            stats = dict(llm.stats)
            alone = [llm.generate(prompt_token_ids=[prompts[i]], sampling_params=[sps[i]])[0].outputs[0].token_ids for i in samp_ix]
            gsps = [serving.SamplingParams(temperature=0.0, max_tokens=sps[i].max_tokens, logits_processors=[ban]) for i in range(6)]
            greedy = [o.outputs[0].token_ids for o in llm.generate(prompt_token_ids=prompts, sampling_params=gsps)]
            return mixed, stats, alone, greedy
        for slots in (4, 16):
            res = _threaded([lambda r=r: serve(r, slots) for r in range(2)], grp, timeout=240)
            (m0, st0, a0, g0), (m1, _, a1, g1) = res
            assert m0 == m1 and a0 == a1 and g0 == g1, "logical ranks disagree"
            assert st0["sampled_in_batch"] > 0 and st0["batched_requests"] >= 6, st0
            for i in greedy_ix:
                assert m0[i] == g0[i], (slots, i)
            if slots == 4:           # VALU form: per slot bit-identical with the single-request path
                for j, i in enumerate(samp_ix):
                    assert m0[i] == a0[j], (slots, i)
            assert all(t not in range(100, 400) for o in m0 for t in o)
    finally:
        os.environ.pop("USDM_NO_GRAPH", None)


# ------------------------------------------------------------------------------------------------------------- 4. P2P form
def test_logits_p2p_kernel_split_form(dev):
    """The exchange alone at the 7B's Vloc at TP = 8 (5251 logits: 6 workgroups, 11 sites of 512): rows, status, epoch."""
    from usdm_amd import ops
    from usdm_amd.p2p import P2PComm
    Vloc, me, tp = 5251, 512, 2
    comms = P2PComm.in_process(tp, 2 + -(-Vloc // me), me, timeout_ms=2000)
    g = torch.Generator().manual_seed(1)
    loc = [torch.randn(Vloc, generator=g).to(dev) for _ in range(tp)]
    rows = [torch.zeros(tp * Vloc, device=dev) for _ in range(tp)]
    for it in range(3):
        for r in range(tp):
            ops.logits_p2p(loc[r], Vloc, None, comms[r], 2, rows[r], phase=1)
        for r in range(tp):
            ops.logits_p2p(loc[r], Vloc, None, comms[r], 2, rows[r], phase=2)
        torch.cuda.synchronize()
        want = torch.cat(loc)
        for r in range(tp):
            assert torch.equal(rows[r], want)
            assert comms[r].status() == (0, 2 + it)
        loc = [x + 1 for x in loc]


@pytest.mark.parametrize("tp", [2, 4])
def test_p2p_split_form_equals_collective_form(dev, tp):
    from usdm_amd.p2p import InProcessGroup, P2PComm
    ids = _ids(dev)
    new, (T, k, p), seed = 10, SETTINGS[1], 123
    ref = lockstep_sample(_ranks(dev, tp, InProcessGroup(tp)), ids, new, T, k, p, seed)
    n = P2PComm.sites_needed(CFG, tp, True)
    comms = P2PComm.in_process(tp, n, CFG["hidden_size"], timeout_ms=2000)
    ranks = _ranks(dev, tp, InProcessGroup(tp), comms=comms, p2p_fused=False)
    got = lockstep_sample(ranks, ids, new, T, k, p, seed, oracle=True)
    assert got == ref
    for c in comms:
        assert c.status() == (0, 1 + new)


def test_p2p_fused_form_two_streams_and_site_check(dev):
    from tests._tp_lockstep import lockstep_generate
    from usdm_amd.p2p import InProcessGroup, P2PComm
    tp, new, (T, k, p), seed = 2, 12, SETTINGS[2], 321
    ids = _ids(dev)
    ref = lockstep_sample(_ranks(dev, tp, InProcessGroup(tp)), ids, new, T, k, p, seed)
    comms = P2PComm.in_process(tp, P2PComm.sites_needed(CFG, tp, True), CFG["hidden_size"], timeout_ms=3000)
    grp = InProcessGroup(tp, threaded=True)
    ranks = _ranks(dev, tp, grp, comms=comms, p2p_fused=True)
    os.environ["USDM_NO_GRAPH"] = "1"
    try:
        outs = _threaded([lambda r=r: ranks[r].generate(input_ids=ids, max_new_tokens=new, do_sample=True, temperature=T, top_k=k or None,
                                                         top_p=p, seed=seed, bad_words_ids=BAD)[0, ids.shape[1]:].tolist() for r in range(tp)], grp)
    finally:
        os.environ.pop("USDM_NO_GRAPH", None)
    assert outs[0] == outs[1] == ref
    for c in comms:
        assert c.status() == (0, 1 + new)
    # a communicator sized for the greedy step: greedy still works, sampling names the sites it needs
    small = P2PComm.in_process(tp, 2 * CFG["num_hidden_layers"] + 1, CFG["hidden_size"], timeout_ms=2000)
    sranks = _ranks(dev, tp, InProcessGroup(tp), comms=small, p2p_fused=False)
    lockstep_generate(sranks, ids, 6, bad_words_ids=BAD)
    need = P2PComm.sites_needed(CFG, tp, True)
    with pytest.raises(ValueError, match=f"needs a P2PComm of {need} sites"):
        sranks[0].generate(input_ids=ids, max_new_tokens=4, do_sample=True, temperature=1.0, seed=1)
    for c in small:
        assert c.status()[0] == 0
