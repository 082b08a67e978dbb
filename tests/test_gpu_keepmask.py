"""The keep-mask generator on the GPU (csrc/keepmask.hip through ns_km_draw, smart_nar_fast_tts_amd.dropout, the hooks in _train.py and
training.py).  Everything is bit-equality with tests/keepmask_cpu.py's yardstick, so there is no tolerance.

The kernel alone first: every case of ``keepmask_cpu.CASES`` (single masks of n in {1, 15, 16, 17, 4095, 4096, 4097, 2*7*256, 2*20*80}
at each p, a mixed table, seed >= 2^63 with call >= 2^32 and streams up to 2^32 - 1, a threshold that is one of the mask's words) drawn
into the middle of a canary-filled buffer: the slots, their zero tails and the untouched canaries before, between nothing, and behind;
exactly one launch.  Then the test model's own mask list padded to 40 mixed masks through ``KeepMaskRNG.prefetch``, an arena of more
than NS_KM_GRID_CAP * 4096 elements (workgroups loop), and a short arena (the kernel stops at arena_bytes).

Then the Python layer on train_align_tiny (B 2, L 7, T 20, 1 + 4 layers, dropout as configured) with ``torch.bernoulli`` patched to
raise: the arena path against the module-by-module path and against the yardstick's masks given as ``keep_masks=``, bit for bit in
outputs, losses and every gradient; one draw, no host read; and a run resumed from ``save_checkpoint(..., rng=rng)``."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import keepmask_cpu as kc
from tests import optim_cpu as oc
from tests.util import ROOT, native_lib

pytestmark = pytest.mark.gpu
FRONT, BACK = 64, 80  # canary bytes around the arena


@pytest.fixture(scope="module")
def so():
    return native_lib()


def _table(L, lib, masks):
    n = len(masks)
    arr = (L.NsKmMask * n)()
    for i, (cnt, stream, thr) in enumerate(masks):
        arr[i].n, arr[i].stream, arr[i].thr = cnt, stream, thr
    nbytes = lib.ns_km_table_bytes(n)
    host = np.zeros(nbytes, dtype=np.uint8)
    need = C.c_uint64(0)
    L.check(lib.ns_km_plan(arr, n, host.ctypes.data, nbytes, C.byref(need)), "ns_km_plan")
    return torch.from_numpy(host).cuda(), int(need.value)


def _draw(L, lib, masks, seed, call, arena_bytes=None):
    """the whole canary buffer after one ns_km_draw into its middle, and the planned arena bytes"""
    table, need = _table(L, lib, masks)
    given = need if arena_bytes is None else arena_bytes
    buf = torch.full((FRONT + max(need, given) + BACK,), kc.CANARY, dtype=torch.uint8, device="cuda")
    L.check(lib.ns_km_draw(L.ptr(table), len(masks), seed, call, C.c_void_p(buf.data_ptr() + FRONT), given, L.stream_ptr()), "ns_km_draw")
    assert lib.ns_km_last_launches() == 1
    torch.cuda.synchronize()
    return buf.cpu().numpy(), need


def _framed(want):
    return np.concatenate([np.full(FRONT, kc.CANARY, np.uint8), want, np.full(BACK, kc.CANARY, np.uint8)])


# ---------------------------------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_cases_bit_equal_to_the_yardstick(so, name):
    L, lib = so
    c = kc.CASES[name]
    got, need = _draw(L, lib, c["masks"], c["seed"], c["call"])
    want = kc.case_arena(name)
    assert need == want.size
    assert got.tobytes() == _framed(want).tobytes(), name
    again, _ = _draw(L, lib, c["masks"], c["seed"], c["call"])
    assert again.tobytes() == got.tobytes(), "two draws, equal bits"
    if name in kc.CATCHER.values():  # the mutants this case is there for do differ from what the kernel wrote
        for mutate, where in kc.CATCHER.items():
            if where == name:
                assert _framed(kc.case_arena(name, mutate)).tobytes() != got.tobytes(), mutate


def test_a_short_arena_is_cut_and_never_overrun(so):
    L, lib = so
    c = kc.CASES["mixed"]
    want = kc.case_arena("mixed")
    short = want.size - 4096 - 16  # ends inside the last-but-one slot: whole 16-byte groups before it are written, nothing from it on
    got, need = _draw(L, lib, c["masks"], c["seed"], c["call"], arena_bytes=short)
    assert need == want.size
    assert got[:FRONT + short].tobytes() == _framed(want)[:FRONT + short].tobytes()
    assert (got[FRONT + short:] == kc.CANARY).all()


def test_workgroups_loop_past_the_grid_cap(so):
    L, lib = so
    big = L.KM_GRID_CAP * 4096 + 4097  # more chunks than workgroups: every workgroup takes a second chunk, some a third
    masks = [(4100, 3, kc.threshold(0.1)), (big, 4, kc.threshold(0.2)), (17, 5, kc.threshold(0.5))]
    got, need = _draw(L, lib, masks, 1234, 9)
    want = kc.arena(masks, 1234, 9)
    assert need == want.size > L.KM_GRID_CAP * 4096
    assert np.array_equal(got, _framed(want))


def _tiny_model():
    from tests import test_gpu_train_align as ta

    meta, z, (pcfg, cfg), sd, batch = ta._tiny()
    # the fixture's config has dropout 0 (its reference step has none): the ljspeech values, as tests/test_gpu_train_align.py sets them
    cfg = dict(cfg, transformer=dict(cfg["transformer"], encoder_dropout=0.2, decoder_dropout=0.2), variance_predictor=dict(cfg["variance_predictor"], dropout=0.5))
    return ta, meta, pcfg, cfg, sd, batch


def test_the_models_list_in_one_table(so):
    """the test model's own masks, padded with further shapes to 40, through KeepMaskRNG.prefetch and take"""
    from smart_nar_fast_tts_amd import dropout

    ta, meta, pcfg, cfg, sd, _ = _tiny_model()
    m = ta._build(pcfg, cfg, sd).train()
    entries = m._step_masks({}, meta["B"], meta["L"], meta["T"], meta["T"])
    t = cfg["transformer"]
    assert len(entries) == 2 * t["encoder_layer"] + 1 + 4 * t["decoder_layer"] + 6 + 5
    extra = [((1, 1, 1), 0.5), ((3, 5, 7), 0.1), ((2, 33, 256), 0.2), ((1, 4097, 1), 0.5), ((2, 2, 2048), 0.2), ((1, 15, 1), 0.1)]
    entries = (entries + extra * 7)[:40]
    assert len(entries) == 40
    rng = dropout.KeepMaskRNG((1 << 63) + 11)
    rng.call = (1 << 32) + 4
    rng.next_call()
    rng.prefetch(entries, torch.device("cuda"))
    assert rng.launches == 1
    for i, (shape, p) in enumerate(entries):
        (got,) = rng.take([shape], p, torch.device("cuda"))
        assert got.dtype == torch.uint8 and tuple(got.shape) == shape and got.data_ptr() % 16 == 0 and got.is_contiguous()
        want = kc.mask(rng.seed, rng.call, i, int(np.prod(shape)), kc.threshold(p))
        assert np.array_equal(got.cpu().numpy().reshape(-1), want), (i, shape, p)
    assert rng.launches == 1 and rng.stream == 40
    # past the arena a take draws for itself, at the next streams; the same (shape, p) list again is the cached table
    a, b = rng.take([(2, 3, 4), (2, 3, 4)], 0.5, torch.device("cuda"))
    assert rng.launches == 2 and rng.stream == 42
    for i, got in ((40, a), (41, b)):
        assert np.array_equal(got.cpu().numpy().reshape(-1), kc.mask(rng.seed, rng.call, i, 24, kc.threshold(0.5)))
    # a take that is not what the arena has next raises, naming both
    rng.next_call()
    rng.prefetch(entries[:3], torch.device("cuda"))
    with pytest.raises(RuntimeError, match=r"asked for \(\(\(9, 9, 9\), 0.2\),\).*has"):
        rng.take([(9, 9, 9)], 0.2, torch.device("cuda"))


# ---------------------------------------------------------------------------------------------------- the Python layer
def _given(m, entries, seed, call):
    """the yardstick's masks of ``entries`` (streams 0, 1, ...) as the ``keep_masks=`` dict of training.FastSpeech2Align"""
    from tests.util import dev

    it = iter(dev(kc.mask(seed, call, i, int(np.prod(s)), kc.threshold(p)).reshape(s)) for i, (s, p) in enumerate(entries))
    pair = lambda: [next(it), next(it)]  # noqa: E731
    km = {"txt_encoder": [pair() for _ in m.txt_encoder.layer_stack], "prenet": next(it), "mel_encoder": [pair() for _ in m.mel_encoder.layer_stack]}
    va = m.variance_adaptor
    km["variance_adaptor"] = {"duration": pair()}
    for level in ("phoneme_level", "frame_level"):
        for name, lv in (("pitch", va.pitch_feature_level), ("energy", va.energy_feature_level)):
            if lv == level:
                km["variance_adaptor"][name] = pair()
    km["mel_decoder"] = [pair() for _ in m.mel_decoder.layer_stack]
    km["postnet"] = [next(it) for _ in m.postnet.channels[1:]]
    assert next(it, None) is None
    return km


def test_model_arena_path_module_path_and_given_masks_agree(monkeypatch):
    from smart_nar_fast_tts_amd import dropout
    from smart_nar_fast_tts_amd.loss import FastSpeech2TrainingLoss

    ta, meta, pcfg, cfg, sd, batch = _tiny_model()
    m = ta._build(pcfg, cfg, sd).train()
    loss = FastSpeech2TrainingLoss(pcfg, cfg)
    spec = importlib.util.spec_from_file_location("_ns_tools_bench", os.path.join(ROOT, "tools", "_bench.py"))
    tb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tb)
    bn = ta._bn_state(m)

    def no_bernoulli(*a, **k):
        raise AssertionError("torch.bernoulli must not run with a generator attached")

    monkeypatch.setattr(torch, "bernoulli", no_bernoulli)
    entries = m._step_masks({}, meta["B"], meta["L"], meta["T"], meta["T"])
    assert len(entries) >= 30 and all(0.0 < p < 1.0 for _, p in entries)

    def run(seed, prefetch=True, given=None, count_reads=False):
        m.load_state_dict(bn, strict=False)
        ta._clear(m)
        rng = None
        if given is None:
            rng = dropout.KeepMaskRNG(seed)
            dropout.attach(m, rng)
        else:
            dropout.detach(m)
        m.prefetch_keep_masks = prefetch
        res = {}

        def step():
            res["out"] = m(*batch[2:], keep_masks=given)
            res["seven"] = loss(batch, res["out"])
            res["seven"][0].backward()

        if count_reads:
            torch.cuda.synchronize()
            res["reads"] = tb.host_reads(step)
        else:
            step()
        torch.cuda.synchronize()
        res["seven"] = torch.stack(list(res["seven"])).detach().cpu().numpy().view(np.uint32)
        res["flat"], res["grads"], res["rng"], res["last"] = ta._flat(res.pop("out")), ta._grads(m), rng, dict(m.last_launches)
        return res

    def same(a, b, what):
        assert np.array_equal(a["seven"], b["seven"]), (what, "the seven losses")
        for i, (p, q) in enumerate(zip(a["flat"], b["flat"])):
            if isinstance(p, list):
                assert all(np.array_equal(x, y) for x, y in zip(p, q)), (what, "maps", i)
            else:
                assert np.array_equal(p, q), (what, "tuple entry", i)
        assert a["grads"].keys() == b["grads"].keys()
        for n in a["grads"]:
            assert (a["grads"][n] is None) == (b["grads"][n] is None) and (a["grads"][n] is None or np.array_equal(a["grads"][n], b["grads"][n])), (what, n)

    try:
        run(7)  # (a warm-up: the layers' workspace caches fill; the counted run below still uploads its own generator's table)
        arena = run(1234, count_reads=True)
        assert arena["reads"][0] == 0, arena["reads"][1]
        assert arena["rng"].launches == 1 and arena["rng"].state_dict() == {"version": 1, "seed": 1234, "call": 1, "stream": len(entries)}
        by_module = run(1234, prefetch=False)
        # one draw per layer that has dropout (a predictor's two masks and the PostNet's five are one draw each)
        sites = len(entries) - 3 - (len(m.postnet.channels) - 2)
        assert by_module["rng"].launches == sites > 1 and by_module["rng"].stream == len(entries)
        assert by_module["last"]["forward"] == arena["last"]["forward"] + sites - 1 and by_module["last"]["backward"] == arena["last"]["backward"]
        same(arena, by_module, "arena path against module-by-module path")
        given = run(None, given=_given(m, entries, 1234, 1))
        assert given["last"]["forward"] == arena["last"]["forward"] - 1, "launches include the draw"
        same(arena, given, "arena path against the yardstick's masks as keep_masks=")
        same(arena, run(1234), "two identical runs")
        other = run(1235)
        assert not np.array_equal(other["seven"], arena["seven"]) and not np.array_equal(other["flat"][0], arena["flat"][0])
        a, b = dropout.KeepMaskRNG(1234), dropout.KeepMaskRNG(1235)
        for r in (a, b):
            r.next_call()
        s, p = entries[0]
        assert not torch.equal(a.take([s], p, torch.device("cuda"))[0], b.take([s], p, torch.device("cuda"))[0])
        # a second step draws other masks: the call counter moved
        rng = dropout.KeepMaskRNG(1234)
        dropout.attach(m, rng)
        m.prefetch_keep_masks = True
        with torch.no_grad():
            one = ta._flat(m(*batch[2:]))
            two = ta._flat(m(*batch[2:]))
        assert rng.call == 2 and not np.array_equal(one[0], two[0]) and np.array_equal(one[0], arena["flat"][0])
        # eval(): no draw, no call consumed
        m.eval()
        with torch.no_grad():
            m(*batch[2:])
        assert rng.call == 2 and rng.launches == 2
    finally:
        m.train()
        dropout.detach(m)
        m.prefetch_keep_masks = True
        ta._clear(m)


def test_resumed_run_is_bit_identical(tmp_path, monkeypatch):
    from smart_nar_fast_tts_amd import dropout, optim, training
    from smart_nar_fast_tts_amd.loss import FastSpeech2TrainingLoss

    ta, meta, pcfg, cfg, sd, batch = _tiny_model()
    loss = FastSpeech2TrainingLoss(pcfg, cfg)
    mcfg = {"transformer": {"encoder_hidden": oc.ENCODER_HIDDEN}}
    monkeypatch.setattr(torch, "bernoulli", lambda *a, **k: (_ for _ in ()).throw(AssertionError("torch.bernoulli must not run")))

    def fresh(restore_step):
        m = ta._build(pcfg, cfg, sd).train()
        return m, optim.ScheduledOptim(m, ta.OCFG, mcfg, restore_step), dropout.KeepMaskRNG(99)

    m, opt, rng = fresh(0)
    dropout.attach(m, rng)
    for step in (1, 2):
        training.train_step(m, loss, opt, batch, step, 1, oc.GRAD_CLIP)
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in m.state_dict().items()}
    assert rng.call == 2

    m1, opt1, rng1 = fresh(0)
    dropout.attach(m1, rng1)
    training.train_step(m1, loss, opt1, batch, 1, 1, oc.GRAD_CLIP)
    path = str(tmp_path / "1.pth.tar")
    training.save_checkpoint(m1, opt1, path, rng=rng1)
    del m1, opt1, rng1
    ckpt = torch.load(path, map_location="cuda", weights_only=True)
    assert sorted(ckpt) == ["keep_mask_rng", "model", "optimizer"] and ckpt["keep_mask_rng"] == {"version": 1, "seed": 99, "call": 1, "stream": rng.stream}
    m2, opt2, rng2 = fresh(1)
    rng2.seed = 0  # (everything comes from the file)
    m2.load_state_dict(ckpt["model"], strict=True)
    opt2.load_state_dict(ckpt["optimizer"])
    rng2.load_state_dict(ckpt["keep_mask_rng"])
    dropout.attach(m2, rng2)
    training.train_step(m2, loss, opt2, batch, 2, 1, oc.GRAD_CLIP)
    torch.cuda.synchronize()
    got = m2.state_dict()
    assert list(got) == list(want)
    for k, v in want.items():
        assert torch.equal(v, got[k]), k
    assert rng2.state_dict() == rng.state_dict()
    moved = [k for k in want if want[k].dtype == torch.float32 and not torch.equal(want[k].cpu(), torch.as_tensor(np.asarray(sd[k])))]
    assert len(moved) > 50, "the two steps moved the parameters"
