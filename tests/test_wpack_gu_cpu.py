"""CPU: the packer of the lossless 13-bit weight image (usdm_amd/wpack.py) on an interleaved gate/up matrix (blocks of 16 gate + 16
up rows; PackedWeight.from_matrix(w, glu=True)): the rows come back bit for bit, the bitmap of the kernel argument is per OUTPUT
(its gate row or its up row marked) and agrees with a plain loop over gemv_glu_row's formula, an inf and a NaN mark their rows
without lifting the window off the bulk, and the limit is N / 2 <= 14336 outputs."""
import pytest
import torch

BF = torch.bfloat16
K = 4096


def _bits(w):
    return w.view(torch.int16).to(torch.int32) & 0xffff


def _from_bits(b):
    return b.to(torch.int16).view(BF)


def _gate_up(nout, seed):
    from usdm_amd.llm import _pack_gate_up
    g = torch.Generator().manual_seed(seed)
    Wg, Wu = ((torch.randn((nout, K), generator=g) * K ** -0.5).to(BF) for _ in range(2))
    W = _pack_gate_up(Wg, Wu)
    W[W.abs() < 2.0 ** -20] = 2.0 ** -9          # (the draw's own tiny weights: only the planted rows are marked)
    return W


def _glu_row(o, up):        # csrc/gemv_common.h gemv_glu_row, written out
    return (o >> 4) * 32 + (o & 15) + (16 if up else 0)


def test_round_trip_and_bits_per_output():
    from usdm_amd import wpack
    nout = 48
    b = _bits(_gate_up(nout, 11)).clone()
    # (output, up?) -> bits: gate only, up only, both rows of one output, the first and the last output, a block's last gate row
    plant = {(0, False): 0x0000, (5, True): 0x8000, (17, False): 0x0001, (17, True): 0x0080, (31, False): 0x0000, (47, True): 0x8000}
    for i, ((o, up), v) in enumerate(plant.items()):
        assert wpack.glu_row(o, up) == _glu_row(o, up)
        b[_glu_row(o, up), (131 * i + 7) % K] = v
    W = _from_bits(b)
    p = wpack.PackedWeight.from_matrix(W, glu=True)
    assert p.glu and (p.N, p.K) == (2 * nout, K) and p.planes.shape == (2 * nout, 2 * 3328)
    assert p.marked_rows == sorted(_glu_row(o, up) for o, up in plant)
    keep = [r for r in range(2 * nout) if r not in p.marked_rows]
    assert torch.equal(wpack.unpack(p.planes, p.base, K)[keep], b[keep])
    # the bitmap against a plain loop over the formula
    flag = p.rowflag.tolist()
    want = [o for o in range(nout) if flag[_glu_row(o, False)] or flag[_glu_row(o, True)]]
    assert want == sorted({o for o, _ in plant}) == p.marked_outputs
    a = p.args()
    assert a.units == 2 and a.stride == 2 * 3328 and len(a.marked) == 448
    got = [o for o in range(32 * 448) if a.marked[o >> 5] >> (o & 31) & 1]
    assert got == want
    # the same matrix taken as plain rows keeps one bit per row
    q = wpack.PackedWeight.from_matrix(W)
    assert not q.glu and q.marked_outputs is None and q.marked_rows == p.marked_rows
    rows = [r for r in range(32 * 448) if q.args().marked[r >> 5] >> (r & 31) & 1]
    assert rows == p.marked_rows


def test_inf_and_nan_mark_their_rows_and_leave_the_window():
    from usdm_amd import wpack
    nout = 32
    b = _bits(_gate_up(nout, 12)).clone()
    top = int(((b >> 8) & 0x7f).max())
    b[_glu_row(3, False), 100] = 0x7f80      # +inf in a gate row
    b[_glu_row(20, True), 200] = 0x7fc0      # NaN in an up row
    b[_glu_row(9, True), 300] = 0x7000       # a huge weight in an up row
    p = wpack.PackedWeight.from_matrix(_from_bits(b), glu=True)
    assert p.base == top - 15                 # the window stays on the bulk
    assert p.marked_outputs == [3, 9, 20] and p.marked_rows == sorted((_glu_row(3, False), _glu_row(20, True), _glu_row(9, True)))
    keep = [r for r in range(2 * nout) if r not in p.marked_rows]
    assert torch.equal(wpack.unpack(p.planes, p.base, K)[keep], b[keep])


def test_the_limit_is_on_outputs():
    from usdm_amd import wpack
    planes = torch.zeros((2 * wpack.MAX_ROWS, 8), dtype=torch.uint8)       # (the constructor looks at the row count only)
    flag = torch.zeros(2 * wpack.MAX_ROWS, dtype=torch.uint8)
    flag[2 * wpack.MAX_ROWS - 1] = 1                                        # the last up row -> the last output
    p = wpack.PackedWeight(planes, flag, 100, K, glu=True)
    assert p.marked_outputs == [wpack.MAX_ROWS - 1] and p.args().marked[447] == 1 << 31
    with pytest.raises(ValueError):
        wpack.PackedWeight(planes, flag, 100, K)                            # as plain rows: twice the limit
    more = torch.zeros((2 * wpack.MAX_ROWS + 32, 8), dtype=torch.uint8)
    with pytest.raises(ValueError):
        wpack.PackedWeight(more, torch.zeros(2 * wpack.MAX_ROWS + 32, dtype=torch.uint8), 100, K, glu=True)
    with pytest.raises(ValueError):
        wpack.PackedWeight(planes[:48], flag[:48], 100, K, glu=True)        # not whole blocks of 16 gate + 16 up rows
