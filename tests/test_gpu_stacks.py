"""The trainable TxtEncoder and MelDecoder on the GPU (csrc/stackgrad.hip through ns_st_* and stacks.py).

The two new kernels alone first.  The table gradient against the float64 sum at the derived bound of tests/stacks_cpu.py
(``embed_grad_bound``: 0.5 ulp32(|s|) + n_hits 2^-53 sum |g|), with PAD and unused rows checked as +0.0 by their bits, two runs bit-equal,
and — because that bound holds for any order of the float64 adds — the bits of ``embed_grad_ordered``, the ascending order replayed on
the CPU (the "order" case is built so that another order gives other bits).  The row mask bit-equal to ``np.where`` forward and backward,
in its mask and its lens form.  The two forward ops bit-equal to the numpy fp32 add.

Then the stacks at d 256, H 2, d_inner 256, 2 layers, B, S = 3, 33, lens [33, 1, 32], in train() at p = 0.5 with given keep-masks: every
bit of the output and of every gradient equal to the hand chain (the op, then FFTBlock x 2, the table gradient taken by the op alone from
the chain's dx), the launch counts include/nar_fs2.h states, and eval() outputs against the float64 statement at the project gate.
Gradients are judged by bit-equality with the chain only: the chain's kernels are each held to float64 alone in their own test files,
and a ReLU pre-activation within a rounding of zero can change sign in float64, which is a property of the input.

With a frozen embedding the stack's own backward launch (the table gradient) is gone, exactly one; the whole count falls by two,
because layer 0's attention then drops its own dx launch by its needs_input_grad rule.  The test asserts both.

NS_FP32_OPS_REPORT=<path> appends every measured share as a JSON line (profiles/stacks_grad.md is written from one).

Measured on the MI355X (profiles/stacks_grad.md): every bit-equality holds; the table gradient is inside its bound on all 40 cases; the
eval() outputs are at 0.27 (encoder) and 0.29 (decoder) of the gate, the native step at 0.24 of optim_cpu.gate_of."""
import numpy as np
import pytest
import torch

from tests import attention_grad_cpu as ac
from tests import ffn_grad_cpu as fc
from tests import optim_cpu as oc
from tests import stacks_cpu as sc
from tests.util import dev, gate_value, native_lib, report, share_of

pytestmark = pytest.mark.gpu
D, H, DI, KS, NL, B, S, LENS, P = 256, 2, 256, (9, 1), 2, 3, 33, [33, 1, 32], 0.5
N_VOCAB = 361


@pytest.fixture(scope="module")
def so():
    return native_lib()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------------- the table gradient alone
@pytest.mark.parametrize("case", sc.EMBED_CASES)
@pytest.mark.parametrize("dims", sc.EMBED_DIMS, ids=lambda d: f"d{d[0]}v{d[1]}")
def test_embed_grad_alone(so, dims, case):
    L, lib = so
    Dd, V = dims
    g, t = sc.embed_case(case, Dd, V)
    M = len(t)
    s, bound = sc.embed_grad64(g, t, V), sc.embed_grad_bound(g, t, V)
    runs = []
    for _ in range(2):
        g_d, t_d = dev(g), dev(t)
        out = torch.full((V, Dd), float("nan"), device="cuda")
        L.check(lib.ns_st_op_embed_grad(L.ptr(g_d), L.ptr(t_d), M, Dd, V, L.ptr(out), L.stream_ptr()), "ns_st_op_embed_grad")
        assert lib.ns_st_last_launches() == 1
        runs.append(out.cpu().numpy())
    got = runs[0]
    assert np.isfinite(got).all(), "a NaN of g at a PAD or out-of-range row reached the table"
    err = np.abs(got.astype(np.float64) - s)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"embed_grad {dims} {case}: worst share of the bound {worst:.3g}")
    assert (err <= bound).all(), (case, worst)
    unused = np.ones(V, dtype=bool)
    unused[t[(t >= 1) & (t < V)]] = False
    assert unused[0] and not got[unused].view(np.uint32).any(), "PAD and unused rows are +0.0 by their bits"
    assert np.array_equal(got.view(np.uint32), sc.embed_grad_ordered(g, t, V).view(np.uint32)), "float64 adds in ascending m, rounded once"
    assert np.array_equal(got.view(np.uint32), runs[1].view(np.uint32)), "two runs are bit-equal"


# ---------------------------------------------------------------------------------------------------- the row mask alone
MASK_CASES = [(3, 33, [33, 1, 32]), (1, 1, [1]), (1, 1, [0]), (2, 70, [0, 70])]


@pytest.mark.parametrize("width", [256, 512])
@pytest.mark.parametrize("case", MASK_CASES, ids=lambda c: f"{c[0]}x{c[1]}_{'_'.join(map(str, c[2]))}")
def test_row_mask_alone(so, case, width):
    from smart_nar_fast_tts_amd import stacks

    Bc, Sc, lens = case
    rs = np.random.RandomState(Bc * Sc + width)
    pad = sc.pad_of(lens, Sc)
    x = rs.standard_normal((Bc, Sc, width)).astype(np.float32)
    g = rs.standard_normal((Bc, Sc, width)).astype(np.float32)
    x[pad], g[pad] = np.nan, np.nan
    want_y, want_dx = sc.mask_rows(x, pad), sc.mask_rows(g, pad)
    assert np.isfinite(want_y).all() and not want_y[pad].view(np.uint32).any()
    got = {}
    for form, kw in (("mask", dict(mask=dev(pad))), ("lens", dict(lens=dev(np.asarray(lens, dtype=np.int64)))),
                     ("both", dict(mask=dev(pad), lens=dev(np.full(Bc, Sc, dtype=np.int64))))):  # both: the mask is used
        xd = dev(x).requires_grad_(True)
        book = stacks.Launches()
        y = stacks.mask_rows(xd, book=book, **kw)
        y.backward(dev(g))
        assert book.last == {"forward": 1, "backward": 1}
        got[form] = (_bits(y), _bits(xd.grad))
        assert np.array_equal(got[form][0], want_y.view(np.uint32)), form
        assert np.array_equal(got[form][1], want_dx.view(np.uint32)), form
        with torch.no_grad():
            assert np.array_equal(_bits(stacks.mask_rows(dev(x), **kw)), want_y.view(np.uint32))
    assert all(np.array_equal(got["mask"][i], got[f][i]) for f in ("lens", "both") for i in (0, 1))


# ---------------------------------------------------------------------------------------------------- the forward ops
@pytest.mark.parametrize("width", [256, 512])
def test_forward_ops_equal_the_numpy_add(so, width):
    L, lib = so
    Bc, Sc, V = 3, 33, 11
    rs = np.random.RandomState(width)
    emb = rs.standard_normal((V, width)).astype(np.float32)
    pos = rs.standard_normal((Sc + 2, width)).astype(np.float32)
    texts = rs.randint(0, V, size=(Bc, Sc)).astype(np.int64)
    texts[0, 0], texts[1, 3], texts[2, 32] = -1, V, 0  # outside [0, V): read as PAD
    x = rs.standard_normal((Bc, Sc, width)).astype(np.float32)
    out = torch.full((Bc, Sc, width), float("nan"), device="cuda")
    e_d, p_d, t_d, x_d = dev(emb), dev(pos), dev(texts), dev(x)
    L.check(lib.ns_st_op_embed_pos(L.ptr(t_d), L.ptr(e_d), L.ptr(p_d), Bc, Sc, width, V, L.ptr(out), L.stream_ptr()), "ns_st_op_embed_pos")
    assert lib.ns_st_last_launches() == 1
    safe = np.where((texts < 0) | (texts >= V), 0, texts)
    assert np.array_equal(_bits(out), (emb[safe] + pos[None, :Sc]).view(np.uint32))
    out.fill_(float("nan"))
    L.check(lib.ns_st_op_add_pos(L.ptr(x_d), L.ptr(p_d), Bc, Sc, width, L.ptr(out), L.stream_ptr()), "ns_st_op_add_pos")
    assert lib.ns_st_last_launches() == 1
    assert np.array_equal(_bits(out), (x + pos[None, :Sc]).view(np.uint32))


# ---------------------------------------------------------------------------------------------------- the stacks
def _config(max_seq_len=40, dropout=P):
    t = dict(conv_filter_size=DI, conv_kernel_size=list(KS))
    for side in ("encoder", "decoder"):
        t.update({f"{side}_hidden": D, f"{side}_head": H, f"{side}_layer": NL, f"{side}_dropout": dropout})
    return {"max_seq_len": max_seq_len, "transformer": t}


def _state_dict(w):
    from smart_nar_fast_tts_amd import sublayers

    sd = {}
    if w["emb"] is not None:
        sd["src_word_emb.weight"] = torch.from_numpy(w["emb"])
    for i, (wa, wf) in enumerate(w["layers"]):
        sd.update({f"layer_stack.{i}.slf_attn.{n}": torch.from_numpy(wa[k]) for n, k in zip(sublayers.PARAM_NAMES, ac.NAMES[:10])})
        sd.update({f"layer_stack.{i}.pos_ffn.{n}": torch.from_numpy(wf[k]) for n, k in zip(sublayers.FFN_PARAM_NAMES, fc.NAMES[:6])})
    return sd


_BUILT = {}


def _stack(kind, max_seq_len=40):
    """(module on the GPU, its seeded weights), built once per (kind, max_seq_len)"""
    from smart_nar_fast_tts_amd import stacks

    key = (kind, max_seq_len)
    if key not in _BUILT:
        enc = kind == "encoder"
        w = sc.seeded_stack(D, DI, KS, NL, seed=400 if enc else 500, n_vocab=N_VOCAB if enc else None)
        m = stacks.TxtEncoder(_config(max_seq_len)) if enc else stacks.MelDecoder(_config(max_seq_len))
        missing = m.load_state_dict(_state_dict(w), strict=False)
        assert missing.missing_keys == ["position_enc"] and not missing.unexpected_keys
        _BUILT[key] = (m.cuda(), w)
    return _BUILT[key]


def _inputs(kind, Bc=B, Sc=S, lens=LENS, seed=0):
    rs = np.random.RandomState(900 + seed + Sc)
    pad = sc.pad_of(lens, Sc)
    if kind == "encoder":
        inp = rs.randint(1, N_VOCAB, size=(Bc, Sc)).astype(np.int64)
        inp[pad] = 0
        inp[0, 3], inp[0, 7] = inp[0, 1], N_VOCAB - 1  # one id twice in an utterance; the last id
    else:
        inp = rs.standard_normal((Bc, Sc, D)).astype(np.float32)
    g = rs.standard_normal((Bc, Sc, D)).astype(np.float32)  # random on every row, padded ones too
    keeps = [[dev((rs.rand(Bc, Sc, D) >= P).astype(np.uint8)) for _ in range(2)] for _ in range(NL)]
    return inp, g, keeps, dev(pad), dev(np.asarray(lens, dtype=np.int64))


def _clear(m):
    for p in m.parameters():
        p.grad = None


def _grads(m):
    return {n: None if p.grad is None else _bits(p.grad) for n, p in m.named_parameters()}


def _run_stack(kind, m, inp, g, keeps, mask, lens):
    """forward + backward through the module: (y bits, {parameter: grad bits}, dx bits or None, last_launches)"""
    _clear(m)
    xin = dev(inp)
    if kind == "decoder":
        xin.requires_grad_(True)
    y = m(xin, mask, lens=lens, keep_masks=keeps)
    y = y if kind == "encoder" else y[0]
    y.backward(dev(g)[:, :y.shape[1]].contiguous())
    return _bits(y), _grads(m), None if kind == "encoder" else _bits(xin.grad), m.last_launches


def _run_chain(kind, m, L, lib, inp, g, keeps, mask, lens, pos=None):
    """the hand chain: the op, FFTBlock x n with the same arguments, the table gradient by the op alone from the chain's dx"""
    _clear(m)
    Bc, Sc = inp.shape[:2]
    pos = m.position_enc.detach()[0] if pos is None else pos
    x0 = torch.empty((Bc, Sc, D), device="cuda")
    xin = dev(inp)
    if kind == "encoder":
        L.check(lib.ns_st_op_embed_pos(L.ptr(xin), L.ptr(m.src_word_emb.weight.detach()), L.ptr(pos), Bc, Sc, D, N_VOCAB, L.ptr(x0), L.stream_ptr()),
                "ns_st_op_embed_pos")
    else:
        L.check(lib.ns_st_op_add_pos(L.ptr(xin), L.ptr(pos), Bc, Sc, D, L.ptr(x0), L.stream_ptr()), "ns_st_op_add_pos")
    x0.requires_grad_(True)
    y = x0
    for i, layer in enumerate(m.layer_stack):
        y, _ = layer(y, mask=mask, lens=lens, keep_masks=None if keeps is None else keeps[i])
    y.backward(dev(g))
    grads = _grads(m)
    if kind == "encoder":
        dw = torch.full((N_VOCAB, D), float("nan"), device="cuda")
        L.check(lib.ns_st_op_embed_grad(L.ptr(x0.grad), L.ptr(xin), Bc * Sc, D, N_VOCAB, L.ptr(dw), L.stream_ptr()), "ns_st_op_embed_grad")
        grads["src_word_emb.weight"] = _bits(dw)
    return _bits(y), grads, None if kind == "encoder" else _bits(x0.grad), None


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), (what, "y")
    assert a[1].keys() == b[1].keys()
    for n in a[1]:
        assert (a[1][n] is None) == (b[1][n] is None) and (a[1][n] is None or np.array_equal(a[1][n], b[1][n])), (what, n)
    assert (a[2] is None) == (b[2] is None) and (a[2] is None or np.array_equal(a[2], b[2])), (what, "dx")


@pytest.mark.parametrize("kind", ["encoder", "decoder"])
def test_stack_equals_the_hand_chain(so, kind):
    L, lib = so
    m, _ = _stack(kind)
    m.train()
    inp, g, keeps, mask, lens = _inputs(kind)
    try:
        before = m.launches
        got = _run_stack(kind, m, inp, g, keeps, mask, lens)
        spent = m.launches - before
        own, a0 = (m.src_word_emb.last_launches, m.layer_stack[0].slf_attn.last_launches["backward"]) if kind == "encoder" else (None, None)
        want = _run_chain(kind, m, L, lib, inp, g, keeps, mask, lens)
        _same(got, want, "stack vs chain")
        y = got[0].view(np.float32)
        pad = mask.cpu().numpy()
        assert np.isfinite(y).all() and not got[0][pad].any() and np.abs(y[~pad]).max() > 0, "padded rows of the output are +0.0 by their bits"
        assert got[1]["position_enc"] is None
        assert all(v is not None for n, v in got[1].items() if n != "position_enc")
        if kind == "encoder":
            assert not got[1]["src_word_emb.weight"][0].any(), "the PAD row of the table gradient is +0.0"
        else:
            assert np.abs(got[2].view(np.float32)).max() > 0
        # the launch counts of include/nar_fs2.h, from the sublayers' own counters
        fwd = 1 + sum(ly.slf_attn.last_launches["forward"] + 1 + ly.pos_ffn.last_launches["forward"] + 1 for ly in m.layer_stack)
        bwd = sum(1 + ly.pos_ffn.last_launches["backward"] + 1 + ly.slf_attn.last_launches["backward"] for ly in m.layer_stack) + (kind == "encoder")
        assert got[3] == {"forward": fwd, "backward": bwd} and spent == fwd + bwd, (got[3], fwd, bwd, spent)
        # the mask alone (lengths derived and validated: one host read) gives the same bits
        _same(_run_stack(kind, m, inp, g, keeps, mask, None), got, "mask alone")
        # the no_grad forward
        with torch.no_grad():
            y0 = m(dev(inp), mask, lens=lens, keep_masks=keeps)
        assert np.array_equal(_bits(y0 if kind == "encoder" else y0[0]), got[0])
        # (a sublayer's no_grad forward may make fewer launches than its saving one: the formula is taken from its counters again)
        fwd0 = 1 + sum(ly.slf_attn.last_launches["forward"] + 1 + ly.pos_ffn.last_launches["forward"] + 1 for ly in m.layer_stack)
        assert m.last_launches == {"forward": fwd0, "backward": 0} and fwd0 <= fwd
        if kind == "encoder":
            # A frozen embedding: the stack's own backward launch (the table gradient) is gone, exactly 1, and there is no gradient.
            # The whole count drops by 2, not 1: nothing upstream of layer 0 wants a gradient any more, so its attention drops its own
            # dx launch by the needs_input_grad rule its header states.  The mirror formula holds with that attention's own count.
            assert own == {"forward": 1, "backward": 1}
            m.src_word_emb.weight.requires_grad_(False)
            frozen = _run_stack(kind, m, inp, g, keeps, mask, lens)
            assert m.src_word_emb.last_launches == {"forward": 1}
            mirror = sum(1 + ly.pos_ffn.last_launches["backward"] + 1 + ly.slf_attn.last_launches["backward"] for ly in m.layer_stack)
            dropped_by_attention = a0 - m.layer_stack[0].slf_attn.last_launches["backward"]
            print(f"frozen embedding: backward {bwd} -> {frozen[3]['backward']} (table gradient 1, layer 0's attention {dropped_by_attention})")
            assert frozen[3] == {"forward": fwd, "backward": mirror} and mirror == bwd - 1 - dropped_by_attention and dropped_by_attention >= 1
            assert frozen[1]["src_word_emb.weight"] is None
            assert np.array_equal(frozen[0], got[0]) and all(np.array_equal(frozen[1][n], got[1][n]) for n in got[1] if "layer_stack" in n)
    finally:
        if kind == "encoder":
            m.src_word_emb.weight.requires_grad_(True)
        _clear(m)


@pytest.mark.parametrize("kind", ["encoder", "decoder"])
def test_replicas_of_an_utterance_are_bit_equal(kind):
    m, _ = _stack(kind)
    m.train()
    lens = [20, 20, 5]
    inp, g, keeps, mask, lens_d = _inputs(kind, lens=lens, seed=3)
    inp[1], g[1] = inp[0], g[0]
    for pair in keeps:
        for k in pair:
            k[1] = k[0]
    try:
        y, _, dx, _ = _run_stack(kind, m, inp, g, keeps, mask, lens_d)
        assert np.array_equal(y[0], y[1]) and not np.array_equal(y[0], y[2])
        if dx is not None:
            assert np.array_equal(dx[0], dx[1])
    finally:
        _clear(m)


@pytest.mark.parametrize("kind", ["encoder", "decoder"])
def test_forward_against_float64(kind):
    m, w = _stack(kind)
    m.eval()
    inp, _, _, mask, lens = _inputs(kind, seed=5)
    with torch.no_grad():
        y = m(dev(inp), mask, lens=lens)
    y = (y if kind == "encoder" else y[0]).cpu().numpy()
    ref = {}
    for dtype in (torch.float32, torch.float64):
        leaves = sc.leaves_of(w, dtype, None if kind == "encoder" else inp)
        with torch.no_grad():
            ref[dtype] = sc.statement(inp if kind == "encoder" else None, leaves, LENS, H, 40, training=False, dtype=dtype, encoder=kind == "encoder")[0].numpy()
    gate = gate_value(ref[torch.float32], ref[torch.float64])
    share, at = share_of(y, ref[torch.float64], gate)
    report(test="st_forward", kind=kind, shares={"y": share}, gate=gate)
    assert share <= 1.0, (kind, share, at)


# ---------------------------------------------------------------------------------------------------- the decoder past max_seq_len
def test_decoder_truncates_in_train_and_regenerates_in_eval(so):
    from smart_nar_fast_tts_amd import ops

    L, lib = so
    m, _ = _stack("decoder", max_seq_len=16)
    Sc, lens = 20, [20, 3, 18]
    inp, g, keeps, mask, lens_d = _inputs("decoder", Sc=Sc, lens=lens, seed=9)
    try:
        m.train()
        _clear(m)
        xin = dev(inp).requires_grad_(True)
        y, mask_out = m(xin, mask, lens=lens_d, keep_masks=[[k[:, :16].contiguous() for k in pair] for pair in keeps])
        assert tuple(y.shape) == (B, 16, D) and torch.equal(mask_out, mask[:, :16])
        y.backward(dev(g)[:, :16].contiguous())
        got = (_bits(y), _grads(m), _bits(xin.grad[:, :16]), None)
        assert not _bits(xin.grad[:, 16:]).any(), "dx past max_seq_len is exactly 0"
        k16 = [[k[:, :16].contiguous() for k in pair] for pair in keeps]
        want = _run_chain("decoder", m, L, lib, inp[:, :16].copy(), g[:, :16].copy(), k16, mask[:, :16].contiguous(), lens_d.clamp(max=16))
        _same(got, want, "truncated vs chain")
        # eval(): the regenerated table, nothing truncated, one more launch
        m.eval()
        _clear(m)
        xin = dev(inp).requires_grad_(True)
        y, mask_out = m(xin, mask, lens=lens_d)
        assert tuple(y.shape) == (B, Sc, D) and mask_out.data_ptr() == mask.data_ptr()
        y.backward(dev(g))
        got = (_bits(y), _grads(m), _bits(xin.grad), None)
        fwd = 2 + sum(ly.slf_attn.last_launches["forward"] + 1 + ly.pos_ffn.last_launches["forward"] + 1 for ly in m.layer_stack)
        assert m.last_launches["forward"] == fwd
        want = _run_chain("decoder", m, L, lib, inp, g, None, mask, lens_d, pos=ops.sinusoid_table(Sc, D))
        _same(got, want, "regenerated vs chain")
        short = _run_chain("decoder", m, L, lib, inp[:, :16].copy(), g[:, :16].copy(), None, mask[:, :16].contiguous(), lens_d.clamp(max=16))
        assert not np.array_equal(got[0][:, :16], short[0]), "rows past 16 are attended to"
    finally:
        _clear(m)


def test_encoder_past_max_seq_len(so):
    from smart_nar_fast_tts_amd import ops

    L, lib = so
    m, _ = _stack("encoder", max_seq_len=16)
    inp, g, keeps, mask, lens_d = _inputs("encoder", Sc=20, lens=[20, 3, 18], seed=11)
    m.train()
    with pytest.raises(ValueError, match="max_seq_len"):
        m(dev(inp), mask, lens=lens_d)
    m.eval()
    try:
        got = _run_stack("encoder", m, inp, g, None, mask, lens_d)
        want = _run_chain("encoder", m, L, lib, inp, g, None, mask, lens_d, pos=ops.sinusoid_table(20, D))
        _same(got, want, "regenerated vs chain")
    finally:
        _clear(m)


# ---------------------------------------------------------------------------------------------------- one native optimiser step
def test_one_native_training_step():
    """a loss-shaped gradient -> the encoder's backward -> optim.ScheduledOptim.step_and_update_lr(): every updated tensor against
    optim_cpu.run on the DEVICE's own gradients, within optim_cpu.gate_of of the fp32 CPU step.  position_enc has no gradient and is
    passed over: its bits do not move."""
    from smart_nar_fast_tts_amd import optim, stacks

    src, w = _stack("encoder")
    m = stacks.TxtEncoder(_config())
    m.load_state_dict(src.state_dict())
    m = m.cuda().eval()
    inp, target, _, mask, lens_d = _inputs("encoder", seed=13)
    with torch.no_grad():
        y0 = m(dev(inp), mask, lens=lens_d).cpu().numpy()
    g = (np.float32(2.0 / (B * S)) * (y0 - target)).astype(np.float32)  # the gradient of an MSE against a random target
    start = 3998
    ocfg = {"optimizer": dict(betas=list(oc.BETAS), eps=oc.EPS, weight_decay=0.0, **oc.SHIPPED)}
    so_ = optim.ScheduledOptim(m, ocfg, {"transformer": {"encoder_hidden": oc.ENCODER_HIDDEN}}, start)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    assert [n for n, p in m.named_parameters() if not p.requires_grad] == ["position_enc"]
    before = [p.detach().cpu().numpy().reshape(-1).copy() for _, p in named]
    pos_before = _bits(m.position_enc).copy()
    y = m(dev(inp), mask, lens=lens_d)
    y.backward(dev(g))
    assert m.position_enc.grad is None and all(p.grad is not None for _, p in named)
    grads = [p.grad.detach().cpu().numpy().reshape(-1).copy() for _, p in named]
    so_.step_and_update_lr()
    lr = so_._optimizer.param_groups[0]["lr"]
    assert abs(lr - oc.lr_at(start + 1, **oc.SHIPPED)) <= 1e-12 * lr
    got = [p.detach().cpu().numpy().reshape(-1) for _, p in named]
    c = dict(params=before, grads=[grads], lrs=[lr], betas=oc.BETAS, eps=oc.EPS, weight_decay=0.0, max_norm=None)
    p64, p32 = oc.run(c)[0]["p"], oc.torch_run(c)[0]["p"]
    sh = {}
    for (n, _), a, t32, w64 in zip(named, got, p32, p64):
        err = np.abs(a.astype(np.float64) - w64).max()
        sh[n] = float(err / oc.gate_of(t32, w64)) if np.isfinite(err) else float("inf")
    report(test="st_native_step", shares={"worst": max(sh.values())})
    assert max(sh.values()) <= 1.0, sh
    assert np.array_equal(_bits(m.position_enc), pos_before)
    assert any(not np.array_equal(a, b) for a, b in zip(got, before))
