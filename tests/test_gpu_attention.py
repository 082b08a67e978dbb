"""The fused attention kernel alone against a float64 restatement of
transformer/Modules.py:14-25, on inputs chosen to exercise every branch: all d_k the config space allows,
ragged key lengths incl. tile-boundary cases, sequence tails, and score spikes that force the online-softmax
reference point to move at a late key tile (the lazy-rescale branch is data dependent and rare)."""
import pytest
import torch

from tests.attention_cpu import form_of, ref_attention  # noqa: F401  (ref_attention: the float64 yardstick, imported by other tests from here)

pytestmark = pytest.mark.gpu


def launch_form(H, dk, S, B, split_scratch=True):
    """the form (tests/attention_cpu.py: A .. G) and key ranges ops.attention_core(..., split_scratch) takes for this shape, asked of
    the dispatch itself (ns_plan_attention_dense) with the scratch and ticket flag the op hands over"""
    from smart_nar_fast_tts_amd import ops

    _, part, tickets = ops.attention_dense_scratch(B, S, H, dk, split_scratch, True)
    pl = ops.plan_attention_dense(B, S, H, dk, part, tickets)
    return form_of(pl, B, S, H), pl[1]


@pytest.mark.parametrize("H,dk", [(2, 128), (8, 64), (4, 32)])
@pytest.mark.parametrize("S,lens", [(1, [1]), (33, [33, 1, 32]), (128, [128, 97, 64, 5]), (300, [300, 257, 129])])
def test_attention_vs_float64(H, dk, S, lens):
    from smart_nar_fast_tts_amd import ops

    torch.manual_seed(S * 7 + dk)
    B = len(lens)
    # strips throughout: one workgroup per strip up to S = 128, 2 or 3 key-range workgroups merged by the last arriver at S = 300
    assert launch_form(H, dk, S, B) == (("A", 1) if S <= 128 else ("B", 2 if H == 8 else 3))
    qkv = torch.randn(B, S, 3 * H * dk)
    lens_t = torch.tensor(lens)
    got = ops.attention_core(qkv.cuda(), lens_t.cuda(), H).cpu()
    ref = ref_attention(qkv, lens_t, H)
    for b in range(B):  # padded QUERY rows are computed by the reference too: compare all S rows
        err = (got[b].double() - ref[b]).abs().max().item()
        assert err < 2e-5, (b, err)


A5_FORMS = {(2, 128, 100): ("A", 1), (2, 128, 128): ("A", 1), (2, 128, 788): ("B", 4), (2, 128, 1010): ("B", 2), (8, 64, 300): ("B", 2),
            (4, 32, 130): ("B", 2)}


@pytest.mark.parametrize("H,dk,S,lens", [(2, 128, 100, [100]), (2, 128, 128, [128, 97, 64, 5] * 4), (2, 128, 788, [788]), (2, 128, 1010, [1010, 700, 33]),
                                         (8, 64, 300, [300, 257, 129]), (4, 32, 130, [130, 1])])
def test_attention_vs_oracle_a5(H, dk, S, lens):
    """Row a5 against the ORACLE's own restatement of ScaledDotProductAttention (oracle/fs2_oracle.py, the function the
    pinned multi_head_attention goes through; fp32 torch-CPU like the reference), on shapes that take two launch forms, both of
    the strip kernel: without a cross-workgroup merge (S <= 128, form A) and with 2 to 4 key-range workgroups per strip merged by
    the last arriver (form B: the single utterance of T = 788 with 4, three utterances of config 2's T = 1010 with 2 — with the
    scratch this op hands over a batch of three still takes strips, not k_attention).  The k_attention forms are held to float64
    one by one in tests/test_gpu_attention_ops.py.  All S query rows are compared — padded ones are computed by the reference too."""
    from oracle import fs2_oracle as orc
    from smart_nar_fast_tts_amd import ops

    torch.manual_seed(S + dk)
    B, d = len(lens), H * dk
    assert launch_form(H, dk, S, B) == A5_FORMS[(H, dk, S)]
    qkv = torch.randn(B, S, 3 * d)
    lens_t = torch.tensor(lens)
    q, k, v = (qkv[..., i * d:(i + 1) * d].reshape(B, S, H, dk).permute(2, 0, 1, 3).reshape(-1, S, dk) for i in range(3))  # SubLayers.py:42-47
    key_pad = torch.arange(S)[None, :] >= lens_t[:, None]
    ref = orc.scaled_dot_product_attention(q, k, v, key_pad.unsqueeze(1).expand(-1, S, -1).repeat(H, 1, 1), dk)
    ref = ref.view(H, B, S, dk).permute(1, 2, 0, 3).reshape(B, S, d)                                                      # SubLayers.py:52-54
    got = ops.attention_core(qkv.cuda(), lens_t.cuda(), H).cpu()
    err = (got - ref).abs().max().item()
    assert err < 2e-5, err


def test_attention_forced_rescale_late_tile():
    """Spike one key per query block far above the rest at a LATE tile so the reference point must move there;
    also a descending spike pattern (first tile largest) so it must NOT move afterwards."""
    from smart_nar_fast_tts_amd import ops

    torch.manual_seed(3)
    B, S, H, dk = 2, 257, 2, 128
    d = H * dk
    assert launch_form(H, dk, S, B) == ("B", 3)  # (strips, 12 key ranges of one tile: the late key lies in the seventh)
    qkv = torch.randn(B, S, 3 * d) * 0.5
    q, k = qkv[..., :d], qkv[..., d:2 * d]
    # utterance 0: key 200 (tile 6) aligned with every query of head 0 -> score ~ +60 in natural units
    k[0, 200, :dk] = q[0, :, :dk].mean(0) * 0 + 6.0
    q[0, :, :dk] += 1.0
    # utterance 1: key 3 (tile 0) huge for head 1, later tiles tiny
    k[1, 3, dk:] = 8.0
    q[1, :, dk:] = q[1, :, dk:].abs() + 0.5
    lens_t = torch.tensor([257, 230])
    got = ops.attention_core(qkv.cuda(), lens_t.cuda(), H).cpu()
    ref = ref_attention(qkv, lens_t, H)
    err = (got.double() - ref).abs().max().item()
    assert err < 5e-5, err
    assert torch.isfinite(got).all()


def test_attention_zero_length_gives_nan_like_reference():
    """An utterance with no valid key: softmax over all -inf is NaN in the reference (SURVEY.md §8b Errors)."""
    from smart_nar_fast_tts_amd import ops

    assert launch_form(2, 128, 40, 2) == ("A", 1)
    qkv = torch.randn(2, 40, 3 * 256)
    got = ops.attention_core(qkv.cuda(), torch.tensor([0, 40]).cuda(), 2).cpu()
    assert torch.isnan(got[0]).all()
    assert torch.isfinite(got[1]).all()


# S -> (form with the op's default scratch, form without scratch)
SPLIT_FORMS = {1000: (("B", 4), ("D", 1)), 700: (("B", 3), ("D", 1)), 513: (("B", 2), ("D", 1)), 260: (("B", 3), ("A", 1))}


@pytest.mark.parametrize("H,dk,S,lens", [(2, 128, 1000, [1000]), (2, 128, 700, [700, 130]), (8, 64, 513, [384]), (4, 32, 260, [260, 31, 0])])
def test_attention_split_key_path(H, dk, S, lens):
    """Few workgroups + long key axis (single-utterance latency) splits the key sweep: with scratch these shapes take the strip
    kernel with 2 to 4 key-range workgroups per strip, merged by the last arriver (form B: partials + ticketed merge, no merge
    launch); without it k_attention in one sweep (form D) three times and unsplit strips (form A) once.  The split must agree with
    float64 and, to rounding, with the single sweep on the same input — incl. ranges that own no valid key tile at all (short
    utterance beside a long one) and the all-masked NaN case.  (k_attention's own splits with the k_attention_merge launch, forms
    E and G, and the strips' merge launch, form C: tests/test_gpu_attention_ops.py.)"""
    from smart_nar_fast_tts_amd import ops

    torch.manual_seed(S + dk)
    B = len(lens)
    assert (launch_form(H, dk, S, B, True), launch_form(H, dk, S, B, False)) == SPLIT_FORMS[S]
    qkv = torch.randn(B, S, 3 * H * dk)
    qkv[0, S // 2 + 7, H * dk:2 * H * dk] *= 4.0  # a dominant key in a late split: weights differ a lot between partials
    lens_t = torch.tensor(lens)
    split = ops.attention_core(qkv.cuda(), lens_t.cuda(), H, split_scratch=True).cpu()
    single = ops.attention_core(qkv.cuda(), lens_t.cuda(), H, split_scratch=False).cpu()
    ref = ref_attention(qkv, lens_t, H)
    for b in range(B):
        if lens[b] == 0:
            assert torch.isnan(split[b]).all() and torch.isnan(single[b]).all()
            continue
        assert (split[b].double() - ref[b]).abs().max().item() < 2e-5
        assert (split[b] - single[b]).abs().max().item() < 1e-5
