#!/usr/bin/env python3
"""Golden outputs and gradients of the two FFT-block stacks — runs ONLY where the reference is checked out (make_golden_aligner.REF; the
import recipe of make_golden_aligner.py).  It imports the reference's ``transformer.Models.TxtEncoder`` and ``MelDecoder``, builds them
with both dropouts 0.0, loads seeded weights (tests/stacks_cpu.seeded_stack) and runs the forward, then ``(g * y).sum().backward()`` in
``train()`` — once in fp32 and once with the same weights and inputs cast to float64 — plus one ``eval()`` forward each.

Config: d = 32, H = 2, d_inner = 64, kernel sizes (3, 1), 2 layers, max_seq_len = 12; B = 4, lens [9, 1, 5, 9] at S = 9.  The decoder
also runs at S = 15 > 12 with lens [15, 1, 5, 13]: in ``train()`` the reference truncates to 12 rows, in ``eval()`` it adds the
regenerated table and keeps all 15.

    python tests/golden/make_golden_stacks.py

stacks_tiny.npz    per case c: {c}_in (texts or x), {c}_g, {c}_y and the gradients of the reference's own autograd as {c}_d_* (fp32) and
                   {c}_d_*_f64, under tests/stacks_cpu.grad_names.  enc: every gradient; dec and dec_trunc: dx (it passes through every layer);
                   enc_eval, dec_eval, dec_long_eval: y only.  The weights are not stored: the meta record holds the seeds.  The
                   reference's state-dict names and shapes are in the meta record too.
"""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_aligner as mga  # noqa: E402  (sets up sys.path and the stub modules the reference's imports need)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden_attention_grad import KEYS as ATTN_KEYS  # noqa: E402
from make_golden_ffn_grad import KEYS as FFN_KEYS  # noqa: E402
from tests import attention_grad_cpu as ac  # noqa: E402
from tests import ffn_grad_cpu as fc  # noqa: E402
from tests import stacks_cpu as sc  # noqa: E402

B, S, LENS, D, D_HID, H, KS, N_LAYERS, MAX_SEQ_LEN = 4, 9, [9, 1, 5, 9], 32, 64, 2, (3, 1), 2, 12
S_LONG, LENS_LONG = 15, [15, 1, 5, 13]
SEEDS = {"encoder": 210, "decoder": 240}


def config():
    t = dict(conv_filter_size=D_HID, conv_kernel_size=list(KS))
    for side in ("encoder", "decoder"):
        t.update({f"{side}_hidden": D, f"{side}_head": H, f"{side}_layer": N_LAYERS, f"{side}_dropout": 0.0})
    return {"max_seq_len": MAX_SEQ_LEN, "transformer": t}


def state_dict(w, table):
    sd = {"position_enc": torch.from_numpy(table.copy())[None]}
    if w["emb"] is not None:
        sd["src_word_emb.weight"] = torch.from_numpy(w["emb"])
    for i, (wa, wf) in enumerate(w["layers"]):
        sd.update({f"layer_stack.{i}.slf_attn.{ATTN_KEYS[k]}": torch.as_tensor(np.asarray(v)) for k, v in wa.items()})
        sd.update({f"layer_stack.{i}.pos_ffn.{FFN_KEYS[k]}": torch.as_tensor(np.asarray(v)) for k, v in wf.items()})
    return sd


def grads_of(m, xt):
    named = dict(m.named_parameters())
    out = {}
    if "src_word_emb.weight" in named:
        out["emb"] = named["src_word_emb.weight"].grad
    if xt is not None:
        out["dx"] = xt.grad
    for i in range(N_LAYERS):
        out.update({f"L{i}_a_{k}": named[f"layer_stack.{i}.slf_attn.{ATTN_KEYS[k]}"].grad for k in ac.NAMES[:10]})
        out.update({f"L{i}_f_{k}": named[f"layer_stack.{i}.pos_ffn.{FFN_KEYS[k]}"].grad for k in fc.NAMES[:6]})
    return out


def record(arrays, c, ref, inp, lens, g, training, keep):
    """one case in fp32 and float64; ``keep`` filters the gradient names that are stored (None: forward only)"""
    Sc = inp.shape[1]
    mask = torch.as_tensor(sc.pad_of(lens, Sc))
    arrays[f"{c}_in"] = inp
    for suffix, dtype in (("", torch.float32), ("_f64", torch.float64)):
        m = copy.deepcopy(ref).to(dtype).train(training)
        xt = None
        if inp.dtype == np.int64:
            y = m(torch.from_numpy(inp), mask)
        else:
            xt = torch.from_numpy(inp).to(dtype).requires_grad_(True)
            y, mask_out = m(xt, mask)
            assert mask_out.shape[1] == y.shape[1]
        assert y.dtype == dtype
        arrays[f"{c}_y{suffix}"] = y.detach().numpy()
        if keep is None:
            continue
        arrays[f"{c}_g"] = g
        (torch.from_numpy(g).to(dtype)[:, :y.shape[1]] * y).sum().backward()
        for name, t in grads_of(m, xt).items():
            if keep(name):
                arrays[f"{c}_d_{name}{suffix}"] = t.numpy()


def make():
    from text.symbols import symbols
    from transformer.Models import MelDecoder, TxtEncoder  # the reference classes

    import smart_nar_fast_tts_amd.workload as wl

    n_vocab = len(symbols) + 1
    assert n_vocab == wl.N_SYMBOLS + 1
    cfg = config()
    table = wl.sinusoid_table(MAX_SEQ_LEN + 1, D)
    arrays, names = {}, {}
    w_enc = sc.seeded_stack(D, D_HID, KS, N_LAYERS, SEEDS["encoder"], n_vocab=n_vocab)
    w_dec = sc.seeded_stack(D, D_HID, KS, N_LAYERS, SEEDS["decoder"])
    enc, dec = TxtEncoder(cfg), MelDecoder(cfg)
    for key, m, w in (("txt_encoder", enc, w_enc), ("mel_decoder", dec, w_dec)):
        names[key] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert np.array_equal(m.position_enc.detach().numpy()[0], table), "workload.sinusoid_table holds the reference's bits"
        m.load_state_dict(state_dict(w, table))
    rs = np.random.RandomState(260)
    texts = rs.randint(1, n_vocab, size=(B, S)).astype(np.int64)
    texts[sc.pad_of(LENS, S)] = 0
    texts[0, 4], texts[3, 2] = texts[0, 1], texts[0, 1]  # one id three times: its table row sums three gradient rows
    x = rs.standard_normal((B, S, D)).astype(np.float32)
    x_long = rs.standard_normal((B, S_LONG, D)).astype(np.float32)
    g = rs.standard_normal((B, S, D)).astype(np.float32)
    g_long = rs.standard_normal((B, S_LONG, D)).astype(np.float32)
    record(arrays, "enc", enc, texts, LENS, g, True, lambda n: True)
    record(arrays, "enc_eval", enc, texts, LENS, g, False, None)
    record(arrays, "dec", dec, x, LENS, g, True, lambda n: n == "dx")
    record(arrays, "dec_eval", dec, x, LENS, g, False, None)
    record(arrays, "dec_trunc", dec, x_long, LENS_LONG, g_long, True, lambda n: n == "dx")
    record(arrays, "dec_long_eval", dec, x_long, LENS_LONG, g_long, False, None)
    assert arrays["dec_trunc_y"].shape == (B, MAX_SEQ_LEN, D) and arrays["dec_long_eval_y"].shape == (B, S_LONG, D)
    assert not arrays["dec_trunc_d_dx"][:, MAX_SEQ_LEN:].any()
    mga.save("stacks_tiny", dict(B=B, S=S, lens=LENS, S_long=S_LONG, lens_long=LENS_LONG, d=D, d_hid=D_HID, H=H, kernel=list(KS), n_layers=N_LAYERS,
                                 max_seq_len=MAX_SEQ_LEN, n_vocab=n_vocab, seeds=dict(SEEDS), state_dict=names), **arrays)


if __name__ == "__main__":
    make()
