"""The training loss on the GPU (csrc/lossgrad.hip through loss.FastSpeech2TrainingLoss): the reference's own backward on the stored
fixtures, seeded tuples at every shape where the kernel takes another path against the float64 closed form (tests/lossgrad_cpu.py)
within the gate, the seven values bit for bit against the value-only class, NaN poison behind every mask and in the gradient
buffers, empty selections, needs_input_grad and null outputs, bitwise determinism, accumulation, the refusals, and the chain into
optim.ScheduledOptim."""
import numpy as np
import pytest
import torch

import smart_nar_fast_tts_amd.workload as wl
from tests import loss_cpu as lc
from tests import lossgrad_cpu as lg
from tests import optim_cpu as oc
from tests.util import load_golden

pytestmark = pytest.mark.gpu


def _loss(level, training=True):
    from smart_nar_fast_tts_amd.loss import FastSpeech2Loss, FastSpeech2TrainingLoss

    cls = FastSpeech2TrainingLoss if training else FastSpeech2Loss
    return cls(wl.preprocess_config(level, level), wl.model_config("tiny"))


def _cuda(x):
    if torch.is_tensor(x):
        return x.cuda()
    return [a.cuda() for a in x] if isinstance(x, (list, tuple)) else x


def _upload(inputs, predictions, grad=True):
    """Device copies of the two tuples; with ``grad`` the nine differentiated tensors are fresh leaves.  Returns (inputs, predictions, nine)."""
    gi, gp = tuple(_cuda(x) for x in inputs), tuple(_cuda(x) for x in predictions)
    leaves = [t.detach().clone().requires_grad_(grad) for t in lg.nine(gp)]
    gp = tuple(leaves[:5]) + gp[5:10] + (leaves[5:], gp[11])
    return gi, gp, leaves


def _seven(out):
    assert len(out) == 7 and all(o.dim() == 0 and o.dtype == torch.float32 and o.is_cuda for o in out)
    assert all(o._base is out[0]._base for o in out) and tuple(out[0]._base.shape) == (7,)
    return out[0]._base


def _run(loss, inputs, predictions, g):
    """(seven values, nine gradients) as numpy arrays: torch.autograd.grad of the seven views with grad_outputs = g."""
    gi, gp, leaves = _upload(inputs, predictions)
    out = loss(gi, gp)
    base = _seven(out)
    gs = torch.as_tensor(np.asarray(g, dtype=np.float32)).cuda()
    grads = torch.autograd.grad(list(out), leaves, grad_outputs=[gs[i] for i in range(7)])
    for x, d in zip(leaves, grads):
        assert d.shape == x.shape and d.dtype == torch.float32 and d.is_contiguous() and d.device == x.device
    return base.detach().cpu().numpy(), [d.cpu().numpy() for d in grads]


def _inside(got, want, gates, what):
    share, where = lg.shares(got, want, gates)
    print(what, "share of the gate:", dict(zip(lg.NAMES, share.round(4))))
    bad = {n: (s, np.unravel_index(w, a.shape), a.flat[w], b.flat[w]) for n, s, w, a, b in zip(lg.NAMES, share, where, got, want) if not s <= 1.0}
    assert not bad, (what, "tensor: (share, element, got, want)", bad)
    return share


def _bits(arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


@pytest.mark.parametrize("name,source", [("lossgrad_tiny", "teacher_tiny"), ("lossgrad_tiny_phoneme_level", "teacher_tiny_phoneme_level")])
def test_fixtures(name, source):
    """total.backward() (train.py:88) against the reference's own float64 backward, the gate from the reference's own fp32 backward."""
    meta, z = load_golden(name)
    ms, zs = load_golden(source)
    inputs, predictions = lc.fixture_case(zs, ms, "")
    gi, gp, leaves = _upload(inputs, predictions)
    out = _loss(ms["pitch"])(gi, gp)
    out[0].backward()
    ref32, ref64 = [z[n] for n in lg.NAMES], [z[n + "_f64"] for n in lg.NAMES]
    gates = lg.gate(ref32, ref64, lg.G_TOTAL, lg.n_attn_of(inputs, predictions))
    _inside([x.grad.cpu().numpy() for x in leaves], ref64, gates, name)
    _, zl = load_golden(name.replace("lossgrad", "loss"))
    values = _seven(out).detach().cpu().numpy()
    assert np.allclose(values, zl["values"], rtol=1e-5, atol=0), (values, zl["values"])


@pytest.mark.parametrize("level", lc.LEVELS)
@pytest.mark.parametrize("name", list(lc.CASES))
def test_random_tuples(name, level):
    inputs, predictions, g, want, gates, _, _, _ = lg.case(name, level)
    _, got = _run(_loss(level), inputs, predictions, g)
    _inside(got, want, gates, f"{name} {level}")


@pytest.mark.parametrize("level", lc.LEVELS)
def test_values_are_bitwise_those_of_the_eval_class(level):
    inputs, predictions, g, _, _, _, _, _ = lg.case("L_past_two_strips_H4_longer_targets", level)
    train = _loss(level)
    values, _ = _run(train, inputs, predictions, g)
    gi, gp, _ = _upload(inputs, predictions, grad=False)
    plain = _seven(_loss(level, training=False)(gi, gp)).cpu().numpy()
    assert values.tobytes() == plain.tobytes(), (values, plain)
    # no prediction requires grad / torch.no_grad(): the parent's forward, no autograd node
    for out in (train(gi, gp), train.eval()(gi, gp)):
        assert _seven(out).grad_fn is None and _seven(out).cpu().numpy().tobytes() == plain.tobytes()
    gi, gp, _ = _upload(inputs, predictions)
    with torch.no_grad():
        out = train(gi, gp)
    assert _seven(out).grad_fn is None and not out[0].requires_grad and _seven(out).cpu().numpy().tobytes() == plain.tobytes()


def _direct(loss, inputs, predictions, g, fill=float("nan"), wanted=range(9)):
    """ns_lossg_forward + ns_lossg_backward into buffers of the test's own: one arena pre-filled with ``fill``, the wanted gradients
    carved from it 64 floats apart.  Returns (the nine arrays or None, True if every float between and around them is untouched)."""
    gi, gp, _ = _upload(inputs, predictions, grad=False)
    call = loss._marshal(gi, gp)
    _, record = loss._value_with_record(call)
    sizes = [x.numel() for x in call.nine]
    arena = torch.full((sum(sizes[i] + 3 for i in wanted) // 4 * 4 + 64 * (len(list(wanted)) + 1) + 64,), fill, dtype=torch.float32, device="cuda")
    outs, used, off = [None] * 9, torch.zeros(arena.numel(), dtype=torch.bool, device="cuda"), 64
    for i in wanted:
        outs[i] = arena[off:off + sizes[i]].view(call.nine[i].shape)
        used[off:off + sizes[i]] = True
        off += (sizes[i] + 3) // 4 * 4 + 64
    loss._backward(call, record, torch.as_tensor(np.asarray(g, dtype=np.float32)).cuda(), outs)
    rest = arena[~used].cpu().numpy()
    untouched = bool(np.isnan(rest).all()) if np.isnan(fill) else bool((rest == fill).all())
    return [None if o is None else o.cpu().numpy() for o in outs], untouched


@pytest.mark.parametrize("level", lc.LEVELS)
def test_poison_behind_every_mask_and_in_the_buffers(level):
    name = "unaligned_prime_T_empty_utterances"
    inputs, predictions, g, want, gates, _, _, _ = lg.case(name, level)
    loss = _loss(level)
    v_clean, clean = _run(loss, inputs, predictions, g)
    pi, pp = lc.poison(inputs, predictions, level, level)
    v_dirty, dirty = _run(loss, pi, pp, g)
    assert np.isfinite(v_clean).all() and v_clean.tobytes() == v_dirty.tobytes()
    assert _bits(dirty) == _bits(clean)
    for n, a, hide in zip(lg.NAMES, dirty, lg.hidden(inputs, predictions, level, level)):
        assert np.isfinite(a).all(), n
        assert hide.any() and not a.view(np.uint32)[hide].any(), (n, "a hidden position must hold +0.0 exactly")
    # NaN in the gradient buffers' own storage before the launch: every element is written, nothing around them is
    direct, untouched = _direct(loss, pi, pp, g)
    assert _bits(direct) == _bits(clean) and untouched


def test_empty_selection():
    inputs, predictions = lc.random_case(3, 9, 33, 2, mel_lens=[0, 0, 0], seed=5)
    values, got = _run(_loss("frame_level"), inputs, predictions, lg.G_TOTAL)
    assert np.isnan(values[[0, 1, 2, 3, 4, 6]]).all() and np.isfinite(values[5]), values
    r32 = lg.autograd_ref(inputs, predictions, "frame_level", "frame_level", lg.G_TOTAL, torch.float32)
    r64 = lg.autograd_ref(inputs, predictions, "frame_level", "frame_level", lg.G_TOTAL, torch.float64)
    for n, a in zip(lg.NAMES, got):
        assert np.isfinite(a).all(), n
        assert (n == "log_d") == bool(a.any()), (n, "all zero except the duration gradient")
    _inside(got, lg.closed_form(inputs, predictions, "frame_level", "frame_level", lg.G_TOTAL), lg.gate(r32, r64, lg.G_TOTAL, 0), "mel_lens = [0, 0, 0]")


def test_needs_input_grad_and_null_outputs():
    level = "frame_level"
    inputs, predictions, g, want, gates, _, _, _ = lg.case("unaligned_prime_T_empty_utterances", level)
    loss = _loss(level)
    _, full = _run(loss, inputs, predictions, g)
    # only mel_predictions requires grad: one buffer, one tensor written
    gi, gp, _ = _upload(inputs, predictions, grad=False)
    mel = gp[0].clone().requires_grad_(True)
    seen = []
    inner = loss._backward
    loss._backward = lambda call, record, go, outs: seen.append([o is not None for o in outs]) or inner(call, record, go, outs)
    out = loss(gi, (mel,) + gp[1:])
    gs = torch.as_tensor(g).cuda()
    (gs * _seven(out)).sum().backward()
    loss._backward = inner
    assert seen == [[True] + [False] * 8], seen
    assert mel.grad.cpu().numpy().tobytes() == full[0].tobytes()
    assert all(t.grad is None for t in lg.nine(gp)[1:])
    # through the C ABI: null pointers for all but postnet, log_d and attn[1]; sentinel storage around them stays as it was
    direct, untouched = _direct(loss, inputs, predictions, g, fill=-7.0, wanted=(1, 4, 6))
    assert untouched
    for i in range(9):
        assert (direct[i] is None) == (i not in (1, 4, 6))
        assert direct[i] is None or direct[i].tobytes() == full[i].tobytes(), lg.NAMES[i]
    none, untouched = _direct(loss, inputs, predictions, g, fill=-7.0, wanted=())
    assert untouched and all(o is None for o in none)


def test_determinism():
    level = "frame_level"
    inputs, predictions, g, _, _, _, _, _ = lg.case("L_past_two_strips_H4_longer_targets", level)
    other = lg.case("exact_tiles", level)
    loss = _loss(level)
    v0, first = _run(loss, inputs, predictions, g)
    v1, again = _run(loss, inputs, predictions, g)
    assert v1.tobytes() == v0.tobytes() and _bits(again) == _bits(first)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        v2, second = _run(loss, inputs, predictions, g)
    side.synchronize()
    assert v2.tobytes() == v0.tobytes() and _bits(second) == _bits(first)
    gs = torch.as_tensor(g).cuda()
    for disturb in ("workspace", "another call"):
        gi, gp, leaves = _upload(inputs, predictions)
        out = loss(gi, gp)
        if disturb == "workspace":
            for w in loss._ws.values():
                w.fill_(0xFF)  # every float64 and int64 word of every slot: NaN / -1.  The record is not in there.
        else:
            oi, op, _ = _upload(other[0], other[1])
            _seven(loss(oi, op))  # its own record; it overwrites the shared workspace
        (gs * _seven(out)).sum().backward()
        assert _seven(out).detach().cpu().numpy().tobytes() == v0.tobytes()
        assert _bits([x.grad.cpu().numpy() for x in leaves]) == _bits(first), disturb


def test_accumulation():
    """Two backwards with g / 2 each accumulate in .grad to within one ulp of one backward with g (g / 2 is exact, so are the halved
    coefficients unless they are denormal)."""
    level = "phoneme_level"
    inputs, predictions, g, _, _, _, _, _ = lg.case("unaligned_prime_T_empty_utterances", level)
    loss = _loss(level)
    _, whole = _run(loss, inputs, predictions, g)
    gi, gp, leaves = _upload(inputs, predictions)
    base = _seven(loss(gi, gp))
    half = torch.as_tensor(g).cuda() / 2
    base.backward(half, retain_graph=True)
    base.backward(half)
    for n, x, w in zip(lg.NAMES, leaves, whole):
        a = x.grad.cpu().numpy()
        ulps = np.abs(a.astype(np.float64) - w) / np.spacing(np.abs(w))
        assert np.isfinite(a).all() and ulps.max() <= 1.0, (n, ulps.max())


def test_modes_and_refusals():
    level = "frame_level"
    inputs, predictions, g, _, _, _, _, _ = lg.case("exact_tiles", level)
    loss = _loss(level)
    swap = lambda t, i, v: t[:i] + (v,) + t[i + 1:]  # noqa: E731
    assert loss.train() is loss and loss.training
    v_train, g_train = _run(loss, inputs, predictions, g)
    assert loss.eval() is loss and not loss.training
    v_eval, g_eval = _run(loss, inputs, predictions, g)
    assert v_train.tobytes() == v_eval.tobytes() and _bits(g_train) == _bits(g_eval)
    gi, gp, leaves = _upload(inputs, predictions)
    with pytest.raises(ValueError, match="mel_predictions must be float32"):
        loss(gi, swap(gp, 0, gp[0].detach().double().requires_grad_(True)))
    with pytest.raises(ValueError, match=r"attn\[2\] must be float32"):
        loss(gi, swap(gp, 10, gp[10][:2] + [gp[10][2].detach().half().requires_grad_(True)] + gp[10][3:]))
    with pytest.raises(ValueError, match=r"pitch_predictions must have shape \(2, 256\)"):
        loss(gi, swap(gp, 2, gp[2].detach()[:, :64].requires_grad_(True)))
    with pytest.raises(ValueError, match=r"attn\[3\] must have shape"):
        loss(gi, swap(gp, 10, gp[10][:3] + [gp[10][3].detach()[:, :1].requires_grad_(True)]))
    with pytest.raises(ValueError, match=r"layers 0-3 \(model/loss.py:233-236\); got 2 map"):
        loss(gi, swap(gp, 10, gp[10][:2]))
    for i, name in ((6, "mel_targets"), (9, "pitch_targets"), (10, "energy_targets")):
        with pytest.raises(ValueError, match=rf"{name}\.requires_grad: targets, masks and lengths get no gradient"):
            loss(swap(gi, i, gi[i].clone().requires_grad_(True)), gp)
    # a double backward: the gradients carry no graph of their own, and where the incoming grad_output has one they refuse to follow it
    out = loss(gi, gp)
    (d_mel,) = torch.autograd.grad(out[0], leaves[:1], create_graph=True, retain_graph=True)
    with pytest.raises(RuntimeError, match="does not require grad"):
        d_mel.sum().backward()
    weight = torch.ones((), device="cuda", requires_grad=True)
    (d_mel,) = torch.autograd.grad(out[0] * weight, leaves[:1], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        d_mel.sum().backward()
    # a non-contiguous prediction gets its gradient in its own layout's shape
    odd = gp[0].detach().transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True)
    loss(gi, swap(gp, 0, odd))[0].backward()
    gi2, gp2, leaves2 = _upload(inputs, predictions)
    loss(gi2, gp2)[0].backward()
    assert odd.grad.shape == odd.shape and torch.equal(odd.grad, leaves2[0].grad)
    # the value-only class keeps refusing
    with pytest.raises(NotImplementedError, match="requires_grad: training is out of scope"):
        _loss(level, training=False)(gi, gp)


class _Holder(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.items = torch.nn.ParameterList(params)


def test_chain_into_scheduled_optim():
    """train.py:83-95 with both native ends: our loss value and backward in front, our clip + Adam + schedule behind, over leaf copies of
    the nine predictions as the parameters.  One step at the plateau of the shipped schedule (step 3999, lr about 1e-3, where a wrong
    or missing gradient moves a parameter by thousands of ulps).  The yardstick is the same step computed in float64 from the float64
    closed-form gradients; the bound is the optimiser's own gate (tests/optim_cpu.py): twice torch's fp32 CPU Adam's distance from
    that float64 step plus one ulp.  The first Adam step divides g by |g| + eps, so it is the gradients' signs, zeros and masks that
    this checks; on this fixture the smallest nonzero |l / ilen - t / olen| is 1 / (ilen * olen) > 2e-3, which keeps every nonzero
    clipped map gradient above 1e-8 >> eps = 1e-9, where that quotient no longer depends on the last bits of W."""
    from smart_nar_fast_tts_amd import optim

    ms, zs = load_golden("teacher_tiny")
    inputs, predictions = lc.fixture_case(zs, ms, "")
    gi, gp, _ = _upload(inputs, predictions, grad=False)
    params = [torch.nn.Parameter(t.clone()) for t in lg.nine(gp)]
    cfg = {"optimizer": dict(betas=list(oc.BETAS), eps=oc.EPS, weight_decay=0.0, **oc.SHIPPED)}
    so = optim.ScheduledOptim(_Holder(params), cfg, {"transformer": {"encoder_hidden": oc.ENCODER_HIDDEN}}, 3998)
    loss = _loss(ms["pitch"]).train()
    out = loss(gi, tuple(params[:5]) + gp[5:10] + (params[5:], gp[11]))
    out[0].backward()
    norm = so.step_and_update_lr(grad_clip_thresh=oc.GRAD_CLIP, zero_grad=True)
    grads64 = lg.closed_form(inputs, predictions, ms["pitch"], ms["energy"], lg.G_TOTAL)
    case = dict(params=[np.asarray(t) for t in lg.nine(predictions)], grads=[grads64], lrs=[oc.lr_at(3999, **oc.SHIPPED)], betas=oc.BETAS,
                eps=oc.EPS, weight_decay=0.0, max_norm=oc.GRAD_CLIP)
    assert so._optimizer.param_groups[0]["lr"] == case["lrs"][0]
    want, t32 = oc.run(case)[0], oc.torch_run(case)[0]
    share = {"norm": abs(norm.item() - want["norm"]) / oc.gate_of(t32["norm"], want["norm"])}
    for n, p, w, t in zip(lg.NAMES, params, want["p"], t32["p"]):
        share[n] = float(np.max(np.abs(p.detach().cpu().numpy().astype(np.float64) - w))) / oc.gate_of(t, w)
        assert not p.grad.any(), "zero_grad=True"
    print("one training step, share of the optimiser's gate:", {k: round(v, 4) for k, v in share.items()})
    assert all(v <= 1.0 for v in share.values()), share
    moved = [float(np.max(np.abs(w - np.asarray(x, dtype=np.float64)))) for w, x in zip(want["p"], case["params"])]
    assert min(moved) > 0.5 * case["lrs"][0], "every tensor takes a step of about lr"
