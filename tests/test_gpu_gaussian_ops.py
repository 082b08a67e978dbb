"""The Gaussian length regulator's two kernels alone (csrc/rowops.hip k_gauss_centers / k_gauss_upsample) against the float64
reference of tests/gaussian_cpu.py under its elementwise bounds, which tests/test_gaussian_host.py proves both ways.

  plain form      ns_op_gaussian_upsampling (the reference module: rows past an utterance's own length are NOT zeroed): out and w
                  under the two bounds, s and the centres exact, max_len = T + 37 rows exactly +0.0 — at odd L, the LDS chunk edge and
                  its padded odd tail, three chunks, 17 channel tiles, pauses of 100+ frames, an utterance of zero durations, T = 32 k
                  and 32 k + 1.
  forwards' form  ns_op_gaussian_regulate, the launch of ns_forward_mel (dense grid) and ns_forward_mel_packed (packed rows): live
                  rows carry the plain form's bits, rows at or past own_len and guard rows are exactly +0.0, status, the zeroed
                  ticket words and what lies next to every output.
  determinism     two runs and a replica of utterance 0 placed last give the same bits.

Every output and scratch buffer is pre-filled with 0xFF bytes.  NS_FP32_OPS_REPORT=<path> appends every measured share as a JSON line
(profiles/gaussian_ops.md was written from one).

Measured on the MI355X (profiles/gaussian_ops.md): the weights at most 0.42 of their bound (three LDS chunks; 0.15 at L = 7 and 9), the
output at most 0.21 of its bound (the 100+ frame pauses; 0.20 where 1e-20 takes over, 0.03 ... 0.09 on short durations), the
forwards' dense form 0.048 and packed form 0.065 — each within 0.01 of the CPU emulation's share, most equal to it in four digits."""
import numpy as np
import pytest
import torch

from smart_nar_fast_tts_amd import _lib, ops
from tests import gaussian_cpu as gc
from tests.util import report as _report

pytestmark = pytest.mark.gpu

_CACHE = {}


def ff(*shape, dtype=torch.float32):
    """a device tensor of a 4-byte type, every byte 0xFF"""
    return torch.full(shape, -1, dtype=torch.int32, device="cuda").view(dtype)


def bits(t):
    return t.contiguous().view(torch.int32)


def plain(x, d, T_out=None):
    """ns_op_gaussian_upsampling on pre-filled buffers: (out [B, T_out, D], s [B (L + 1)], w [B, L, T]) on the CPU"""
    lib = _lib.load()
    B, L, D = x.shape
    T = gc.frames(d)
    T_out = T if T_out is None else T_out
    xd, dd = torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda()
    out, s, w = ff(B, T_out, D), ff(B * (L + 1)), ff(B, L, T)
    _lib.check(lib.ns_op_gaussian_upsampling(_lib.ptr(xd), _lib.ptr(dd), B, L, D, T, T_out, _lib.ptr(out), _lib.ptr(s), _lib.ptr(w),
                                             _lib.stream_ptr(xd.device)), "gaussian_upsampling")
    torch.cuda.synchronize()
    return out.cpu(), s.cpu(), w.cpu()


def case(name):
    """(x, d, own_len, float64 reference of the plain form, the plain form's (out, s, w)), computed once per case"""
    if name not in _CACHE:
        x, d, own_len = gc.CASES[name]()
        _CACHE[name] = (x, d, own_len, gc.reference(x, d), plain(x, d))
    return _CACHE[name]


@pytest.mark.parametrize("name", list(gc.CASES))
def test_plain_form_against_float64(name):
    x, d, _, ref, (out, s, w) = case(name)
    B, L, D = x.shape
    T = ref.T
    sw, so = gc.shares(out.numpy(), w.numpy(), ref)
    _report(test="gaussian_ops", form="plain", case=name, T=T, gpu_w=round(sw, 4), gpu_out=round(so, 4))
    assert sw <= 1.0 and so <= 1.0, (name, sw, so)
    c, total = gc.centres(d)
    assert np.array_equal(s[:B].numpy(), total) and np.array_equal(s[B:].numpy().reshape(B, L), c), "sums and centres are exact"
    padded, s2, w2 = plain(x, d, T + 37)
    assert torch.equal(bits(padded[:, :T]), bits(out)) and torch.equal(bits(w2), bits(w)) and torch.equal(bits(s2), bits(s))
    assert (bits(padded[:, T:]) == 0).all(), "pad(output, max_len) rows are exactly +0.0"


def regulate(x, d, own_len, T, p=None, nzero=1000, with_status=True):
    """ns_op_gaussian_regulate on pre-filled buffers; returns (out with one spare row after it, s, status, zero words) on the CPU"""
    B, L, D = x.shape
    rows = p.Mp if p is not None else B * T
    out, s = ff(rows + 1, D), ff(B * (L + 1))
    status = ff(B + 1, dtype=torch.int32) if with_status else None
    zero = ff(nzero + 1, dtype=torch.int32) if nzero else None
    view = out[:rows] if p is not None else out[:rows].view(B, T, D)
    ops.gaussian_regulate(torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(), torch.tensor(own_len, dtype=torch.long, device="cuda"), T, view, s,
                          p=p, status=None if status is None else status[:B], zero=None if zero is None else zero[:nzero], nzero=nzero)
    torch.cuda.synchronize()
    return out.cpu(), s.cpu(), None if status is None else status.cpu(), None if zero is None else zero.cpu()


def expected_status(own_len, T):
    return [(1 if n > T else 0) | (2 if n < 0 else 0) for n in own_len]


def test_forwards_form_dense():
    x, d, own_len, ref, (pout, ps, _) = case("forwards_dense 5x9x24")
    B, L, D = x.shape
    T = ref.T
    assert own_len == [T, 0, T - 33, -1, T + 5]
    out, s, status, zero = regulate(x, d, own_len, T)
    grid = out[:B * T].view(B, T, D)
    for b, lim in enumerate(gc.row_limit(own_len, T)):
        assert torch.equal(bits(grid[b, :lim]), bits(pout[b, :lim])), (b, "a live row differs from the plain form's")
        assert (bits(grid[b, lim:]) == 0).all(), (b, "a row at or past own_len is not exactly +0.0")
    assert (bits(out[B * T:]) == -1).all(), "the row after the grid was written"
    assert torch.equal(bits(s), bits(ps))
    assert status[:B].tolist() == expected_status(own_len, T) == [0, 0, 0, 2, 1] and status[B] == -1
    assert (zero[:-1] == 0).all() and zero[-1] == -1, "exactly the nzero words are zeroed"
    zeroed = gc.reference(x, d, own_len)
    so = gc.share(grid.numpy(), zeroed.out, zeroed.bound_out)
    _report(test="gaussian_ops", form="forwards dense", case="forwards_dense 5x9x24", T=T, gpu_out=round(so, 4))
    assert so <= 1.0
    # status and the ticket words are nullable: the same rows without them
    again = regulate(x, d, own_len, T, nzero=0, with_status=False)[0]
    assert torch.equal(bits(again), bits(out))


def test_forwards_form_packed():
    x, d, own_len, ref, (pout, ps, _) = case("forwards_packed 5x9x24")
    B, L, D = x.shape
    T = ref.T
    p = ops.pack_plan(own_len, T, 2, gc.PACK_GUARD, device="cuda", fill=-1)
    off, win = p.section("off").cpu().tolist(), p.section("win").cpu().tolist()
    assert win == [min(max(n, 0) + gc.PACK_GUARD, T) for n in own_len] and off[B] == p.Mp < B * T
    assert 0 in own_len and 1 in own_len and T in own_len and any(T - gc.PACK_GUARD <= n < T for n in own_len)
    out, s, status, zero = regulate(x, d, own_len, T, p=p, nzero=37)
    for b, lim in enumerate(gc.row_limit(own_len, T)):
        rows = out[off[b]:off[b] + win[b]]
        assert torch.equal(bits(rows[:lim]), bits(pout[b, :lim])), (b, "a live row differs from the plain form's")
        assert (bits(rows[lim:]) == 0).all(), (b, "a guard row is not exactly +0.0")
    assert (bits(out[p.Mp:]) == -1).all(), "the row after Mp was written"
    assert torch.equal(bits(s), bits(ps))
    assert status[:B].tolist() == expected_status(own_len, T) and status[B] == -1
    assert (zero[:-1] == 0).all() and zero[-1] == -1
    grid = torch.zeros(B, T, D)
    for b in range(B):
        grid[b, :win[b]] = out[off[b]:off[b] + win[b]]
    zeroed = gc.reference(x, d, own_len)
    so = gc.share(grid.numpy(), zeroed.out, zeroed.bound_out)
    _report(test="gaussian_ops", form="forwards packed", case="forwards_packed 5x9x24", T=T, Mp=p.Mp, gpu_out=round(so, 4))
    assert so <= 1.0
    with pytest.raises(RuntimeError, match="weight tensor"):
        ops.gaussian_regulate(torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(), torch.tensor(own_len, device="cuda"), T, ff(p.Mp, D),
                              ff(B * (L + 1)), p=p, w=ff(B, L, T))


def test_determinism_and_replica():
    for name in ("three_chunks 2x513x32", "long_durations 1x11x32"):
        x, d, _, _, first = case(name)
        again = plain(x, d)
        for a, b in zip(first, again):
            assert torch.equal(bits(a), bits(b)), name
    x, d, _, _, (out, s, w) = case("T=32k+1 3x10x40")
    xr, dr = np.concatenate([x, x[:1]]), np.concatenate([d, d[:1]])
    out_r, s_r, w_r = plain(xr, dr)
    assert torch.equal(bits(out_r[3]), bits(out_r[0])) and torch.equal(bits(w_r[3]), bits(w_r[0])), "the replica differs from utterance 0"
    assert torch.equal(bits(out_r[:3]), bits(out)) and torch.equal(bits(w_r[:3]), bits(w)), "a fourth utterance changed the first three"
