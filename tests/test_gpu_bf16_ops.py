"""Each kernel of the opt-in "bf16" mel path ALONE on the MI355X against the float64 emulation of tests/bf16_emu.py (the gates
are proven on the CPU in tests/test_bf16_ops_host.py): k_conv_gemm_bf16 through ops.gemm at every layer shape of the ljspeech and
d512 configs, elementwise; its rounding on exact ties; its LayerNorm tile; the BF = true attention kernels through
ops.attention_core(bf16=True) on the parameter lists of tests/test_gpu_attention.py (strip kernel, forms A and B, plus k_attention
in one sweep where a split test withholds the scratch — each asserted below through the dispatch's own plan; the other dense
forms run in bf16 in tests/test_gpu_attention_ops.py).  Every elementwise bound is applied to ONE
contraction whose inputs the test supplies, so no rounding flip of an earlier layer can enter; the attention gate budgets the
flips of its own P explicitly.

Measured on one MI355X (profiles/bf16_ops_r09.md): GEMM worst 0.0092 of its bound over every shape and tile, LayerNorm blocks
worst 0.020 of theirs, attention worst element 1.87 flips of the 3 allowed and at most 1.05 % of (row, head) pairs above the
fp32 tier (cap 5 %).

NS_BF16_OPS_REPORT=<path> appends every measured figure to a JSON-lines file (profiles/bf16_ops_r09.md was written from one)."""
import numpy as np
import pytest
import torch

from tests import bf16_emu as E
from tests.util import reporter, weights_for

pytestmark = pytest.mark.gpu

METAS = {
    "ljspeech": dict(config="ljspeech", weight_seed=0, frames_per_phoneme=8.0, dur_weight_scale=0.25),
    "d512": dict(config="d512", weight_seed=0, frames_per_phoneme=8.0, dur_weight_scale=0.25),
    "tiny": dict(config="tiny", weight_seed=0, frames_per_phoneme=4.0, dur_weight_scale=0.25),
}
SMALL = [(3, 1), (3, 7), (3, 33), (3, 65), (2, 301)]  # (B, S): partial last tiles, taps crossing both edges of every utterance
TILES = {(256, 256), (128, 256), (64, 128), (64, 64)}
# (name, B, S, the tile the planner must give): sizes that take each remaining tile, ljspeech widths
LARGE = [
    ("mel_decoder.layer_stack.0.pos_ffn.w_1", 16, 950, (256, 256)),   # N = 1024, K = 2304, M = 15 200
    ("mel_decoder.layer_stack.0.pos_ffn.w_1", 8, 800, (128, 256)),
    ("mel_decoder.layer_stack.0.pos_ffn.w_1", 4, 400, (64, 128)),
    ("mel_decoder.layer_stack.0.slf_attn.qkv", 20, 1012, (256, 256)),  # N = 768, K = 256
    ("mel_decoder.layer_stack.0.slf_attn.qkv", 10, 850, (128, 256)),
    ("mel_decoder.layer_stack.0.slf_attn.qkv", 4, 550, (64, 128)),
    ("mel_linear", 16, 800, (64, 128)),                                # N = 80: one partial 128-wide tile
    ("postnet.convolutions.1", 31, 983, (256, 256)),                   # N = 512, K = 2560 (the longest), M = 30 473
    ("postnet.convolutions.1", 13, 975, (128, 256)),
    ("postnet.convolutions.1", 4, 800, (64, 128)),
]


_report = reporter("NS_BF16_OPS_REPORT")


def _build(meta, sd_override=None, modes=("fp32", "bf16")):
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    cfg, sd = weights_for(meta)
    if sd_override:
        sd = dict(sd, **sd_override)
    out = []
    for mode in modes:
        m = FastSpeech2Align(wl.preprocess_config(), dict(cfg, matmul=mode)).to("cuda").eval()
        m.load_state_dict(sd)
        out.append(m)
    return cfg, {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, out


_MODELS = {}


def models(config):
    """(cfg, state dict as tensors, fp32 model, bf16 model); one config at a time"""
    if config not in _MODELS:
        _MODELS.clear()
        cfg, sd, (m32, mbf) = _build(METAS[config])
        _MODELS[config] = (cfg, sd, m32, mbf)
    return _MODELS[config]


@pytest.fixture(scope="module", params=["d512", "ljspeech"])  # (ljspeech last: the fixed-config tests below reuse it)
def config(request):
    """module scope: pytest runs the tests of one config together, so each weight set is built once"""
    return request.param


def contraction(cfg, sd, name):
    """(weight [N, Cin, KW], bias [N], activation) of a name ops.gemm accepts, from the checkpoint, as the library packs it: Q | K |
    V stacked, the PostNet's eval BatchNorm folded in float64 and the folded weight stored as fp32"""
    if name == "mel_linear":
        return sd["mel_linear.weight"][:, :, None], sd["mel_linear.bias"], None
    if name.startswith("postnet.convolutions."):
        i = int(name.rsplit(".", 1)[1])
        n = sum(1 for k in sd if k.startswith("postnet.convolutions.") and k.endswith(".0.conv.weight"))
        sc = sd[name + ".1.weight"].double() / torch.sqrt(sd[name + ".1.running_var"].double() + 1e-5)
        w = (sd[name + ".0.conv.weight"].double() * sc[:, None, None]).float()
        b = ((sd[name + ".0.conv.bias"].double() - sd[name + ".1.running_mean"].double()) * sc + sd[name + ".1.bias"].double()).float()
        return w, b, (None if i == n - 1 else "tanh")
    prefix, which = name.rsplit(".", 1)
    if which == "qkv":
        return (torch.cat([sd[f"{prefix}.{k}.weight"] for k in ("w_qs", "w_ks", "w_vs")])[:, :, None],
                torch.cat([sd[f"{prefix}.{k}.bias"] for k in ("w_qs", "w_ks", "w_vs")]), None)
    w = sd[name + ".weight"]
    return (w if w.dim() == 3 else w[:, :, None]), sd[name + ".bias"], ("relu" if which == "w_1" else None)


def gemm_names(cfg, stack="mel_decoder"):
    n_layer = cfg["transformer"]["decoder_layer" if stack == "mel_decoder" else "encoder_layer"]
    names = [f"{stack}.layer_stack.{i}.{s}" for i in range(n_layer) for s in ("slf_attn.qkv", "slf_attn.fc", "pos_ffn.w_1", "pos_ffn.w_2")]
    return names + (["mel_linear"] + [f"postnet.convolutions.{i}" for i in range(5)] if stack == "mel_decoder" else [])


def _x(B, S, C, seed):
    x = torch.from_numpy(np.random.RandomState(seed).standard_normal((B, S, C)).astype(np.float32))
    assert bool((x != 0).any(dim=-1).all())  # non-zero in every row, the rows next to utterance edges included
    return x


def _check_gemm(model, cfg, sd, name, B, S, seed):
    from smart_nar_fast_tts_amd import ops

    w, b, act = contraction(cfg, sd, name)
    x = _x(B, S, w.shape[1], seed)
    got = ops.gemm(model, name, x.cuda()).cpu()
    res = E.gemm_check(got, x, w, b, act=act)
    tile = ops.plan_gemm_bf16(B * S, w.shape[0])
    _report(test="gemm", name=name, Cin=w.shape[1], N=w.shape[0], KW=w.shape[2], B=B, S=S, tile=list(tile), worst_over_bound=res.worst)
    assert res.ok, f"{name} B={B} S={S} tile={tile}: {res}"
    return tile


# ---------------------------------------------------------------------------------------------------- GEMM, every layer shape
def test_gemm_every_contraction_elementwise(config):
    """|gpu - f64 emulation| <= 1.5e-5 * (conv(|bf x|, |bf w|) + |bias|) at every element, every contraction of the bf16 path
    (all decoder layers, mel_linear, the five PostNet layers), B = 3 at S = 1, 7, 33, 65 and B = 2 at S = 301"""
    cfg, sd, _, mbf = models(config)
    assert mbf._cfg.matmul_bf16x3 == 2
    for n, name in enumerate(gemm_names(cfg)):
        for B, S in SMALL:
            _check_gemm(mbf, cfg, sd, name, B, S, seed=1000 * n + S)


@pytest.mark.parametrize("name,B,S,tile", LARGE)
def test_gemm_large_launch_tiles(name, B, S, tile):
    """the 256x256, 128x256 and 64x128 tiles (the small sizes above all take 64x64), each proven through ns_plan_gemm_bf16"""
    from smart_nar_fast_tts_amd import ops

    cfg, sd, _, mbf = models("ljspeech")
    N = contraction(cfg, sd, name)[0].shape[0]
    assert ops.plan_gemm_bf16(B * S, N) == tile, "the planner's thresholds moved: pick a size that takes this tile again"
    assert _check_gemm(mbf, cfg, sd, name, B, S, seed=B * S) == tile


def test_every_tile_is_exercised():
    """a change of the planner's thresholds cannot silently drop a tile from the cases above"""
    from smart_nar_fast_tts_amd import ops

    cfg, sd, _, _ = models("ljspeech")
    seen = {ops.plan_gemm_bf16(B * S, contraction(cfg, sd, name)[0].shape[0]) for name, B, S, _ in LARGE}
    seen |= {ops.plan_gemm_bf16(B * S, contraction(cfg, sd, name)[0].shape[0]) for name in gemm_names(cfg) for B, S in SMALL}
    assert seen == TILES, seen
    for name in ("mel_decoder.layer_stack.0.pos_ffn.w_1", "mel_decoder.layer_stack.0.slf_attn.qkv", "postnet.convolutions.1"):
        assert {t for n, _, _, t in LARGE if n == name} == TILES - {(64, 64)}
    # mel_linear's 80 columns never take a 256-wide tile (the planner keeps those for N > 128): 64x128 is its only other one
    assert {t for n, _, _, t in LARGE if n == "mel_linear"} == {(64, 128)}


def test_gemm_unknown_name_fails_loudly():
    from smart_nar_fast_tts_amd import _lib

    _, _, m32, _ = models("ljspeech")
    x = torch.zeros(1, 4, 256, device="cuda")
    out = torch.zeros(1, 4, 1024, device="cuda")
    for name in ("mel_decoder.layer_stack.0.pos_ffn.w_3", "postnet.convolutions.5", "postnet.convolutions.x", "mel_decoder.layer_stack.9.pos_ffn.w_1", "mel_decoder.layer_stack.1x.pos_ffn.w_1",
                 "mel_decoder.layer_stack..pos_ffn.w_1", "mel_decoder.layer_stack.-0.pos_ffn.w_1", ""):
        rc = m32._lib.ns_op_gemm(m32._h, name.encode(), _lib.ptr(x), 1, 4, _lib.ptr(out), _lib.stream_ptr(x.device))
        assert rc != 0 and m32._lib.ns_last_error(), name
    torch.cuda.synchronize()
    assert bool((out == 0).all())


# ---------------------------------------------------------------------------------------------------- rounding: ties to even
def _f32(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.float32).copy())


def _tie_values(n, seed):
    """fp32 values on and next to bf16 rounding boundaries: exact midpoints with an even and an odd lower neighbour, both signs,
    one fp32 ulp either side of a midpoint, +-0 and a subnormal"""
    rs = np.random.RandomState(seed)
    hi = (rs.randint(0x3C00, 0x4200, size=n).astype(np.uint32)) | (rs.randint(0, 2, size=n).astype(np.uint32) << 15)  # sign | exp | 7 bits
    lo = np.choose(np.arange(n) % 4, [0x8000, 0x8000, 0x8001, 0x7FFF]).astype(np.uint32)
    hi[0::8] &= ~np.uint32(1)  # even lower neighbour: a tie rounds DOWN in magnitude
    hi[1::8] |= np.uint32(1)   # odd: UP
    bits = (hi << 16) | lo
    bits[[1, 4, 7, 10]] = [0x00000000, 0x80000000, 0x00208000, 0x80218000]  # +0, -0, subnormal ties (even / odd lower neighbour)
    return _f32(bits)


def _half_up(t):
    bits = t.contiguous().view(torch.int32).numpy().view(np.uint32)
    return _f32(((bits.astype(np.uint64) + 0x8000) >> 16 << 16).astype(np.uint32)).reshape(t.shape)


def _one_hot_mel_linear(weight):
    cfg, sd, (m,) = _build(METAS["tiny"], {"mel_linear.weight": weight.numpy(), "mel_linear.bias": np.zeros(80, np.float32)}, modes=("bf16",))
    return m


def test_activation_rounding_is_ties_to_even():
    """one-hot bf16-exact weights (column o copies channel 3 o + 1), zero bias, activations on bf16 rounding boundaries: the
    output is the RNE value exactly — not the truncated one, not round-half-up"""
    from smart_nar_fast_tts_amd import ops

    W = torch.zeros(80, 256)
    cols = 3 * torch.arange(80) + 1
    W[torch.arange(80), cols] = 1.0
    m = _one_hot_mel_linear(W)
    B, S = 3, 33
    x = _tie_values(B * S * 256, seed=4).reshape(B, S, 256).contiguous()
    want = E.bf(x)[:, :, cols]
    assert not torch.equal(want, E.bf_trunc(x)[:, :, cols]) and not torch.equal(want, _half_up(x)[:, :, cols])
    got = ops.gemm(m, "mel_linear", x.cuda()).cpu()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} values are not the ties-to-even rounding"


def test_weight_rounding_is_ties_to_even():
    """weights on bf16 rounding boundaries against one-hot activations (row c is channel c): out[c, o] = RNE(W[o, c]) exactly"""
    from smart_nar_fast_tts_amd import ops

    W = _tie_values(80 * 256, seed=3).reshape(80, 256).contiguous()
    m = _one_hot_mel_linear(W)
    x = torch.eye(256).reshape(1, 256, 256)
    want = E.bf(W).T.reshape(1, 256, 80)
    assert not torch.equal(E.bf(W), E.bf_trunc(W)) and not torch.equal(E.bf(W), _half_up(W))
    got = ops.gemm(m, "mel_linear", x.cuda()).cpu()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} values are not the ties-to-even rounding"


# ---------------------------------------------------------------------------------------------------- mode isolation
def test_mode_covers_the_decoder_only_and_fp32_bits_are_the_existing_ops(config):
    from smart_nar_fast_tts_amd import ops

    cfg, sd, m32, mbf = models(config)
    d = cfg["transformer"]["decoder_hidden"]
    B, S = 3, 65
    x = _x(B, S, d, 7).cuda()
    dec, enc = "mel_decoder.layer_stack.1", "txt_encoder.layer_stack.1"
    assert torch.equal(ops.gemm(m32, "mel_linear", x), ops.mel_linear(m32, x))
    assert torch.equal(ops.gemm(m32, dec + ".pos_ffn.w_1", x), ops.ffn_conv1(m32, dec + ".pos_ffn", x))
    assert torch.equal(ops.gemm(m32, enc + ".pos_ffn.w_1", x), ops.ffn_conv1(m32, enc + ".pos_ffn", x))
    for name in gemm_names(cfg, "txt_encoder"):  # an encoder layer of the bf16 model runs fp32
        xin = _x(B, S, ops.gemm_shape(mbf, name)[0], 11).cuda()
        assert torch.equal(ops.gemm(mbf, name, xin), ops.gemm(m32, name, xin)), name
    for name in (dec + ".slf_attn.qkv", dec + ".pos_ffn.w_1", "mel_linear", "postnet.convolutions.0"):  # ... and a decoder one does not
        xin = _x(B, S, ops.gemm_shape(mbf, name)[0], 12).cuda()
        assert not torch.equal(ops.gemm(mbf, name, xin), ops.gemm(m32, name, xin)), name
    qkv = _x(B, S, 3 * d, 13).cuda()
    lens = torch.tensor([65, 40, 1]).cuda()
    H = cfg["transformer"]["decoder_head"]
    assert torch.equal(ops.attention_core(qkv, lens, H, bf16=False), ops.attention_core(qkv, lens, H))
    assert not torch.equal(ops.attention_core(qkv, lens, H, bf16=True), ops.attention_core(qkv, lens, H))


# ---------------------------------------------------------------------------------------------------- LayerNorm epilogue
# (B, S, lens, the 64 x 256 LayerNorm tile is taken at N = 256): 16 x 801 = 12 816 rows is 200 full tiles and a partial last one
LN_SIZES = [(3, 65, [65, 40, 1], False), (2, 301, [301, 77], False),
            (16, 801, [801, 799, 513, 512, 511, 300, 129, 128, 127, 65, 33, 32, 31, 2, 1, 800], True)]


def _ln_form(cfg, B, S, Cin, full_row):
    """which LayerNorm form the launch takes, asked of the library (ns_plan_gemm_bf16_ln), and that it is the one this size is
    here for: a moved threshold must not turn the full-row case into a third plain one unnoticed"""
    from smart_nar_fast_tts_amd import ops

    d = cfg["transformer"]["decoder_hidden"]
    took = ops.plan_gemm_bf16_ln(B * S, d, Cin)
    assert took == (full_row and d == 256), "the LayerNorm tile's threshold moved: pick sizes on both sides of it again"
    return took


def test_layernorm_tile_is_exercised():
    """the 64 x 256 full-row tile is reached by a case of LN_SIZES at the ljspeech width (both blocks), with a partial last tile"""
    from smart_nar_fast_tts_amd import ops

    for Cin in (256, 1024):
        took = [ops.plan_gemm_bf16_ln(B * S, 256, Cin) for B, S, _, _ in LN_SIZES]
        assert took == [full for _, _, _, full in LN_SIZES] and any(t and (B * S) % 64 for t, (B, S, _, _) in zip(took, LN_SIZES))
    assert not any(ops.plan_gemm_bf16_ln(B * S, 512, 512) for B, S, _, _ in LN_SIZES)  # (N = 512 has no such tile)


@pytest.mark.parametrize("B,S,lens,full_row", LN_SIZES, ids=lambda v: None if isinstance(v, list) else str(v))
def test_ffn_layernorm_epilogue(config, B, S, lens, full_row):
    """LayerNorm(w_2(hid) + x) with hid = the GPU's own relu(w_1(x)), so that no rounding flip enters: below the full-row
    threshold (plain bf16 GEMM + k_layernorm) and at M = 12 816 >= it (the 64 x 256 LayerNorm tile at N = 256: 200 full tiles and a partial last one)"""
    from smart_nar_fast_tts_amd import ops

    cfg, sd, _, mbf = models(config)
    d = cfg["transformer"]["decoder_hidden"]
    p = "mel_decoder.layer_stack.0.pos_ffn"
    took = _ln_form(cfg, B, S, cfg["transformer"]["conv_filter_size"], full_row)
    x = _x(B, S, d, S + d)
    hid = ops.gemm(mbf, p + ".w_1", x.cuda())
    got = ops.positionwise_ffn(mbf, p, x.cuda()).cpu()
    w, b, _ = contraction(cfg, sd, p + ".w_2")
    res = E.gemm_ln_check(got, hid.cpu(), w, b, x, sd[p + ".layer_norm.weight"], sd[p + ".layer_norm.bias"])
    _report(test="ffn_ln", config=config, B=B, S=S, full_row_tile=took, worst_over_bound=res.worst)
    assert res.ok, str(res)


@pytest.mark.parametrize("B,S,lens,full_row", LN_SIZES, ids=lambda v: None if isinstance(v, list) else str(v))
def test_attention_block_layernorm_epilogue(config, B, S, lens, full_row):
    """LayerNorm(fc(att) + x) with att = the GPU's own bf16 attention of its own QKV projection (the scratch sized as the
    model's workspace sizes it, so the launch splits its keys the same way)"""
    from smart_nar_fast_tts_amd import ops

    cfg, sd, _, mbf = models(config)
    d, H = cfg["transformer"]["decoder_hidden"], cfg["transformer"]["decoder_head"]
    p = "mel_decoder.layer_stack.0.slf_attn"
    took = _ln_form(cfg, B, S, d, full_row)
    x = _x(B, S, d, S + d + 1)
    lens_t = torch.tensor(lens)
    qkv = ops.gemm(mbf, p + ".qkv", x.cuda())
    att = ops.attention_core(qkv, lens_t.cuda(), H, split_scratch="workspace", bf16=True)
    got = ops.multi_head_attention(mbf, p, x.cuda(), lens_t.cuda()).cpu()
    w, b, _ = contraction(cfg, sd, p + ".fc")
    res = E.gemm_ln_check(got, att.cpu(), w, b, x, sd[p + ".layer_norm.weight"], sd[p + ".layer_norm.bias"])
    _report(test="mha_ln", config=config, B=B, S=S, full_row_tile=took, worst_over_bound=res.worst)
    assert res.ok, str(res)


@pytest.mark.parametrize("B,S,lens,full_row", LN_SIZES, ids=lambda v: None if isinstance(v, list) else str(v))
def test_masked_rows_are_exactly_zero(config, B, S, lens, full_row):
    """the FFT block masks both LayerNorms: rows at t >= lens[b] are exactly zero, and the valid rows are the bits of the two
    blocks run one after the other on the masked intermediate (either LayerNorm form)"""
    from smart_nar_fast_tts_amd import ops

    cfg, sd, _, mbf = models(config)
    d = cfg["transformer"]["decoder_hidden"]
    p = "mel_decoder.layer_stack.0"
    x = _x(B, S, d, S + d + 2).cuda()
    lens_t = torch.tensor(lens).cuda()
    valid = (torch.arange(S, device="cuda")[None, :] < lens_t[:, None])[:, :, None]
    got = ops.fft_block(mbf, p, x, lens_t)
    assert bool((got.masked_select(~valid.expand_as(got)) == 0).all())
    x1 = torch.where(valid, ops.multi_head_attention(mbf, p + ".slf_attn", x, lens_t), torch.zeros((), device="cuda"))
    want = torch.where(valid, ops.positionwise_ffn(mbf, p + ".pos_ffn", x1), torch.zeros((), device="cuda"))
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------- attention, bf16
def _check_attention(qkv, lens, H, label, **kw):
    from smart_nar_fast_tts_amd import ops

    lens_t = torch.tensor(lens)
    got = ops.attention_core(qkv.cuda(), lens_t.cuda(), H, bf16=True, **kw).cpu()
    ref, unit, flip = E.attention_emu(qkv, lens_t, H)
    for b, n in enumerate(lens):  # zero-length utterances give NaN where the fp32 kernel does
        assert bool(torch.isnan(got[b]).all()) if n == 0 else bool(torch.isfinite(got[b]).all()), (b, n)
    res = E.attention_check(got, ref, unit, flip, H)  # all S query rows, the padded ones too
    _report(test="attention", label=label, H=H, dk=qkv.shape[2] // 3 // H, S=qkv.shape[1], lens=list(lens), worst_flips=res.worst_flips,
            worst_over_fp32_tier=res.worst_fp32, pair_share=res.pair_share, **{k: int(v) for k, v in kw.items()})
    assert res.ok, f"{label} H={H} S={qkv.shape[1]} lens={lens}: {res}"
    return got


@pytest.mark.parametrize("H,dk", [(2, 128), (8, 64), (4, 32)])
@pytest.mark.parametrize("S,lens", [(1, [1]), (33, [33, 1, 32]), (128, [128, 97, 64, 5]), (300, [300, 257, 129])])
def test_attention_bf16_vs_float64(H, dk, S, lens):
    from tests.test_gpu_attention import launch_form

    assert launch_form(H, dk, S, len(lens)) == (("A", 1) if S <= 128 else ("B", 2 if H == 8 else 3))
    torch.manual_seed(S * 7 + dk)
    _check_attention(torch.randn(len(lens), S, 3 * H * dk), lens, H, "ragged")


@pytest.mark.parametrize("H,dk,S,lens", [(2, 128, 100, [100]), (2, 128, 128, [128, 97, 64, 5] * 4), (2, 128, 788, [788]), (2, 128, 1010, [1010, 700, 33]),
                                         (8, 64, 300, [300, 257, 129]), (4, 32, 130, [130, 1])])
def test_attention_bf16_launch_forms(H, dk, S, lens):
    """the strip kernel without a merge (S <= 128, form A) and with the ticketed last-arriver merge (form B: one utterance of
    T = 788 in 4 key-range workgroups per strip, three of T = 1010 in 2 — strips too, not k_attention)"""
    from tests.test_gpu_attention import A5_FORMS, launch_form

    assert launch_form(H, dk, S, len(lens)) == A5_FORMS[(H, dk, S)]
    torch.manual_seed(S + dk)
    _check_attention(torch.randn(len(lens), S, 3 * H * dk), lens, H, "launch form")


@pytest.mark.parametrize("H,dk,S,lens", [(2, 128, 1000, [1000]), (2, 128, 700, [700, 130]), (8, 64, 513, [384]), (4, 32, 260, [260, 31, 0])])
def test_attention_bf16_split_key_path(H, dk, S, lens):
    """partials + the last arriver's merge on strips (form B), and the single sweep on the same input (k_attention, form D; unsplit
    strips at S = 260): both inside the gate (every launch form rounds the same P)"""
    from tests.test_gpu_attention import SPLIT_FORMS, launch_form

    assert (launch_form(H, dk, S, len(lens), True), launch_form(H, dk, S, len(lens), False)) == SPLIT_FORMS[S]
    torch.manual_seed(S + dk)
    qkv = torch.randn(len(lens), S, 3 * H * dk)
    qkv[0, S // 2 + 7, H * dk:2 * H * dk] *= 4.0  # a dominant key in a late split
    _check_attention(qkv, lens, H, "split", split_scratch=True)
    _check_attention(qkv, lens, H, "single sweep", split_scratch=False)


def test_attention_bf16_forced_rescale_late_tile():
    """one key far above the rest at a LATE tile (the reference point must move there), and a descending pattern (it must not)"""
    torch.manual_seed(3)
    B, S, H, dk = 2, 257, 2, 128
    d = H * dk
    qkv = torch.randn(B, S, 3 * d) * 0.5
    q, k = qkv[..., :d], qkv[..., d:2 * d]
    k[0, 200, :dk] = 6.0
    q[0, :, :dk] += 1.0
    k[1, 3, dk:] = 8.0
    q[1, :, dk:] = q[1, :, dk:].abs() + 0.5
    _check_attention(qkv, [257, 230], H, "forced rescale")


def test_attention_bf16_zero_length_gives_nan():
    got = _check_attention(torch.randn(2, 40, 3 * 256), [0, 40], 2, "zero length")
    assert torch.isnan(got[0]).all() and torch.isfinite(got[1]).all()
