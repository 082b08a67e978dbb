"""The row-local selection kernels of csrc/rowops.hip ALONE on the MI355X, bit for bit against numpy / torch on the CPU, at sizes where
their loops take a second trip (more than one 256-wide tile, more than one workgroup): k_bucketize, k_duration_scan<SCAN_COUNTS> +
k_length_regulate (ops.length_regulate), k_mask, k_duration_round.  They select and copy; nothing here needs a tolerance — except
k_duration_round, whose expf may differ from torch's exp in the last bit: it is held to torch's bits wherever exp(x) - 1 (float64) is
farther than 1e-5 relative from a rounding half, and to one of the two neighbouring integers elsewhere.  The inputs are checked on
the CPU first (test_*_inputs, no GPU): at most 1 % of the duration_round values are that close to a half."""
import numpy as np
import pytest
import torch

INF = np.float32(np.inf)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------- bucketize
def bucket_case(n, n_edges, seed):
    """(values [n], edges [n_edges]): ascending fp32 edges; values on edges, one fp32 step either side, below / above all edges,
    -0.0, NaN and both infinities first, random ones after; cut to n from a rotating start so that small n still meet specials"""
    rs = np.random.RandomState(seed)
    edges = np.sort(rs.uniform(-3, 3, size=n_edges).astype(np.float32))
    if n_edges > 2:
        edges[n_edges // 2] = 0.0  # an edge at zero: -0.0 and +0.0 fall on it
        edges = np.sort(edges)
    special = np.concatenate([edges, np.nextafter(edges, -INF), np.nextafter(edges, INF),
                              [edges[0] - 1, edges[-1] + 1, -0.0, 0.0, np.nan, INF, -INF]]).astype(np.float32)
    vals = np.concatenate([special, rs.uniform(-3.5, 3.5, size=max(n, 8)).astype(np.float32)])
    start = (7 * seed) % special.size
    vals = np.roll(vals, -start)[:n] if n < special.size else vals[:n]
    return torch.from_numpy(vals.copy()), torch.from_numpy(edges)


BUCKET_CASES = [(n, e) for n in (1, 5, 1027) for e in (1, 63, 64, 65, 255)]


def test_bucketize_inputs():
    v, e = bucket_case(1027, 255, 3)
    assert bool(torch.isin(e, v).all()) and bool(torch.isnan(v).any()) and bool(torch.isinf(v).any())
    assert bool((v < e[0]).any()) and bool((v > e[-1]).any()) and bool(((v == 0) & torch.signbit(v)).any())
    assert torch.bucketize(v, e).unique().numel() == 256


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_edges", BUCKET_CASES)
def test_bucketize_equals_torch(n, n_edges):
    from smart_nar_fast_tts_amd import ops

    v, e = bucket_case(n, n_edges, seed=n + n_edges)
    got = ops.bucketize(v.cuda(), e.cuda()).cpu()
    want = torch.bucketize(v, e, right=False)
    assert got.dtype == torch.long and torch.equal(got, want), (n, n_edges, (got != want).nonzero().flatten().tolist()[:8])


# ---------------------------------------------------------------------------------------------------- length regulator
def duration_case(B, L, seed):
    """[B, L] fp32 durations as LengthRegulator.expand reads them (max(int(d), 0), int() truncating): zeros, fractions, negatives,
    -0.0, small counts; utterance 1 all zero"""
    rs = np.random.RandomState(seed)
    d = rs.randint(0, 5, size=(B, L)).astype(np.float32)
    d += rs.choice([0.0, 0.25, 0.5, 0.99], size=(B, L)).astype(np.float32)
    neg = rs.rand(B, L) < 0.1
    d[neg] = -d[neg] - 0.5
    d[rs.rand(B, L) < 0.05] = -0.0
    if B > 1:
        d[1] = 0.0
    return torch.from_numpy(d)


def regulate_ref(x, d, max_len):
    """numpy.repeat + zero padding / cut to max_len (model/modules.py:201-230, utils/tools.py:288-306)"""
    xn, dn = x.numpy(), d.numpy()
    cnt = np.maximum(dn.astype(np.int64), 0)  # (astype truncates toward zero, like int())
    mel_len = cnt.sum(axis=1)
    T = int(max_len) if max_len else int(mel_len.max())
    out = np.zeros((x.shape[0], T, x.shape[2]), np.float32)
    for b in range(x.shape[0]):
        rows = np.repeat(xn[b], cnt[b], axis=0)[:T]
        out[b, :rows.shape[0]] = rows
    return torch.from_numpy(out), torch.from_numpy(mel_len)


REG_CASES = [(L, 3, D) for L in (1, 255, 256, 257, 600) for D in (4, 256, 260, 512, 1028)]  # (L, B, D)


def test_length_regulate_inputs():
    d = duration_case(3, 600, 5)
    assert bool((d == 0).any()) and bool((d < 0).any()) and bool((d != d.round()).any()) and bool(((d == 0) & torch.signbit(d)).any())
    assert bool((d[1] == 0).all())
    x = torch.arange(3 * 600 * 4, dtype=torch.float32).reshape(3, 600, 4)
    out, mel_len = regulate_ref(x, d, None)
    assert int(mel_len[1]) == 0 and int(mel_len.max()) == out.shape[1] > 600 and int(mel_len.max()) < 2 ** 31
    assert bool((out[1] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("L,B,D", REG_CASES)
def test_length_regulate_equals_numpy_repeat(L, B, D):
    from smart_nar_fast_tts_amd import ops

    d = duration_case(B, L, seed=L + D)
    x = torch.from_numpy(np.random.RandomState(L * D).standard_normal((B, L, D)).astype(np.float32))
    x[0, 0, 0] = -0.0
    _, mel_len = regulate_ref(x, d, None)
    longest = int(mel_len.max())
    for max_len in sorted({None, max(longest - 3, 1), longest, longest + 5} - {0}, key=lambda v: -1 if v is None else v):
        if longest == 0 and max_len is None:
            continue  # (nothing to regulate and no length given)
        want, want_len = regulate_ref(x, d, max_len)
        got, got_len = ops.length_regulate(x.cuda(), d.cuda(), max_len)
        assert got_len.dtype == torch.long and torch.equal(got_len.cpu(), want_len), (L, B, D, max_len)
        assert got.shape == want.shape and torch.equal(_bits(got.cpu()), _bits(want)), (L, B, D, max_len)


# ---------------------------------------------------------------------------------------------------- mask
@pytest.mark.gpu
@pytest.mark.parametrize("max_len", [1, 37, 255, 257, 1031])
def test_mask_from_lengths_equals_comparison(max_len):
    from smart_nar_fast_tts_amd import ops

    lens = torch.tensor([0, max_len, max_len + 3, 1, max_len // 2, max_len - 1, 2 ** 40])
    assert (lens.numel() * max_len) % 256 != 0
    got = ops.mask_from_lengths(lens.cuda(), max_len).cpu()
    want = torch.arange(max_len)[None, :] >= lens[:, None]
    assert got.dtype == torch.bool and got.shape == want.shape and torch.equal(got, want)
    assert bool(got[0].all()) and not bool(got[1].any()) and not bool(got[2].any())


# ---------------------------------------------------------------------------------------------------- duration rounding
HALF_REL = 1e-5
D_CONTROLS = (1.0, 0.5, 1.5)


def round_case():
    """(x [1027] fp32, e = exp(x) - 1 in float64, near: exp(x) - 1 within HALF_REL of a rounding half): log-durations over
    [-6, 6] (exp(x) - 1 up to 402: a window of 1e-5 relative stays narrow against the unit spacing of the halves), x =
    fp32(log(k + 1.5)) for k = 0 ... 3 — exp(x) - 1 an exact half of either parity up to the rounding of exp — and one fp32
    neighbour of each, 0, -0.0, negatives down to e = -1"""
    rs = np.random.RandomState(11)
    halves = np.log(np.arange(4) + 1.5).astype(np.float32)
    special = np.concatenate([halves, np.nextafter(halves[:2], INF), np.nextafter(halves[2:], -INF), [0.0, -0.0, -6.0, 6.0, np.log(0.5) - 0.01, -0.01]])
    x = np.concatenate([special.astype(np.float32), rs.uniform(-6, 6, size=1027 - special.size).astype(np.float32)])
    rs.shuffle(x)
    e = np.expm1(x.astype(np.float64))
    half = np.floor(e) + 0.5
    near = np.abs(e - half) <= HALF_REL * np.abs(half)
    return torch.from_numpy(x), e, near


def test_duration_round_inputs():
    x, e, near = round_case()
    assert x.numel() == 1027 and 8 <= int(near.sum()) <= 0.01 * x.numel()  # the exact halves are among the excluded, nothing else much
    assert bool(((x == 0) & torch.signbit(x)).any()) and bool((x < 0).any())
    k = np.floor(e[near])
    assert {0, 1, 2, 3} <= set(k.astype(int))  # halves of both parities
    # torch's clamp keeps -0.0 (round(exp(x) - 1) = -0.0 for -0.5 < exp(x) - 1 < 0): the kernel's `r < 0 ? 0 : r` does too
    r = torch.clamp(torch.round(torch.exp(x) - 1) * 1.0, min=0)
    assert bool(((r == 0) & torch.signbit(r)).any()) and bool((r > 100).any()) and bool((r >= 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("d_control", D_CONTROLS)
def test_duration_round_equals_torch_away_from_halves(d_control):
    from smart_nar_fast_tts_amd import ops

    x, e, near = round_case()
    got = ops.duration_round(x.cuda(), d_control).cpu()
    want = torch.clamp(torch.round(torch.exp(x) - 1) * d_control, min=0)
    far = torch.from_numpy(~near)
    diff = _bits(got) != _bits(want)
    assert not bool((diff & far).any()), (d_control, x[diff & far][:8].tolist(), got[diff & far][:8].tolist(), want[diff & far][:8].tolist())
    # next to a half: one of the two neighbouring integers, scaled and clamped the same way
    c = torch.tensor(d_control, dtype=torch.float32)
    lo = torch.clamp(torch.from_numpy(np.floor(e)).float() * c, min=0)
    hi = torch.clamp(torch.from_numpy(np.floor(e) + 1).float() * c, min=0)
    nn = torch.from_numpy(near)
    assert bool(((got == lo) | (got == hi))[nn].all())
