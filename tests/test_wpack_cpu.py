"""CPU: the packer of the lossless 13-bit weight image (usdm_amd/wpack.py) against its pure-torch unpack, on the raw bits.
Random weights at the benchmark's scales (randn * K ** -0.5 rounded to bf16) with weights outside the 16-field exponent window
planted in known rows: exactly those rows (and any the random draw itself produces, which are printed) are marked, every other row
comes back bit for bit, the planes have the stated size, and the window sits where the issue's rule puts it (the matrix's largest
ordinary upper-seven-bit exponent - 15) although an inf, a NaN and a huge weight are in the matrix."""
import pytest
import torch

BF = torch.bfloat16


def _bits(w):
    return w.view(torch.int16).to(torch.int32) & 0xffff


def _from_bits(b):
    return b.to(torch.int16).view(BF)


def _random(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((N, K), generator=g) * K ** -0.5).to(BF)


@pytest.mark.parametrize("N,K,seed", [(40, 14336, 0), (64, 4096, 1)])
def test_round_trip_and_marked_rows(N, K, seed):
    from usdm_amd import wpack
    b = _bits(_random(N, K, seed)).clone()
    e7 = (b >> 8) & 0x7f
    top = int(e7.max())
    own = set(torch.nonzero((e7 < top - 15).any(dim=1)).flatten().tolist())
    print(f"{N} x {K}: largest exponent field {top}; rows the random draw alone puts outside the window: {sorted(own)}")
    # +0, -0, a denormal, the smallest normal, the largest magnitude one binade below the window, a weight above it, inf, NaN
    plant = {1: 0x0000, 5: 0x8000, 9: 0x0001, 12: 0x0080, 17: ((top - 16) << 8) | 0xff, 20: 0x7000, 23: 0xff80, 30: 0x7fc0}
    for i, (r, v) in enumerate(plant.items()):
        b[r, (131 * i + 7) % K] = v
    W = _from_bits(b)
    planes, flag, base = wpack.pack(W)
    assert base == top - 15
    assert planes.shape == (N, K // 2048 * 3328) and planes.dtype == torch.uint8
    assert flag.shape == ((N + 3) // 4 * 4,) and flag.dtype == torch.uint8
    marked = set(torch.nonzero(flag[:N]).flatten().tolist())
    print("marked rows:", sorted(marked))
    assert marked == set(plant) | own
    assert N - len(marked) >= N - len(plant) - 1           # the cap: the test cannot pass by marking everything
    keep = [r for r in range(N) if r not in marked]
    assert torch.equal(wpack.unpack(planes, base, K)[keep], b[keep])
    p = wpack.PackedWeight.from_matrix(W)                   # verifies its own round trip
    assert p.marked_rows == sorted(marked) and p.base == base and p.nbytes == planes.numel() + flag.numel()
    assert p.marked_share == len(marked) / N


def test_every_bit_of_a_unit_goes_through():
    """One unit whose 2048 weights hold every low byte, every window index and both signs at changing places"""
    from usdm_amd import wpack
    i = torch.arange(4 * 2048, dtype=torch.int32).view(4, 2048)
    b = ((i * 37 + (i >> 8)) & 0xff) | ((0x30 + ((i * 7 + (i >> 11)) & 15)) << 8) | (((i * 5 + (i >> 4)) & 1) << 15)
    planes, flag, base = wpack.pack(_from_bits(b))
    assert base == 0x30 and not bool(flag.any())
    assert torch.equal(wpack.unpack(planes, base, 2048), b)
    # the stated layout, at one weight: row 2, iteration 3, lane 41, k 6
    e = 512 * 3 + 8 * 41 + 6
    v = int(b[2, e])
    row = planes[2].to(torch.int32)
    assert int(row[1024 + 16 * 41 + 8 * (3 - 2) + 6]) == v & 0xff
    assert (int(row[2048 + 4 * (4 * 41 + 3) + (6 & 3)]) >> 4) == ((v >> 8) & 0x7f) - base
    sd = sum(int(row[3072 + 4 * 41 + j]) << (8 * j) for j in range(4))
    assert (sd >> (8 * (6 & 3) + 7 - (2 * 3 + 1))) & 1 == v >> 15


def test_marked_bits_in_the_kernel_argument():
    from usdm_amd import wpack
    b = _bits(_random(72, 2048, 3)).clone()
    for r in (2, 31, 32, 71):
        b[r, r] = 0
    a = wpack.PackedWeight.from_matrix(_from_bits(b)).args()
    assert a.units == 1 and a.stride == 3328 and len(a.marked) == 448
    assert list(a.marked)[:3] == [1 << 2 | 1 << 31, 1, 1 << 7] and not any(list(a.marked)[3:])
