"""The optimiser step, everything that needs no GPU: the float64 restatement (tests/optim_cpu.py) against the values captured from the
reference's own ScheduledOptim loop, ScheduledOptim's schedule bit for bit, every mutant rejected by the gate, the ns_opt_* C ABI's
host side (version, struct layouts, planner, table builder, every refusal), the plain-C caller, the Python refusals and the kernels'
register hygiene."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from smart_nar_fast_tts_amd import _lib
from tests import optim_cpu as oc
from tests.util import assert_no_spill, load_golden, run_c_caller

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nar_fs2.h")


def unflat(row, case):
    out, o = [], 0
    for p in case["params"]:
        out.append(row[o:o + p.size].reshape(p.shape))
        o += p.size
    return out


def fixture_trajectory(z, tag, key, case):
    return [{"p": unflat(z[f"{tag}_{key}_p"][k], case), "m": unflat(z[f"{tag}_{key}_m"][k], case), "v": unflat(z[f"{tag}_{key}_v"][k], case),
             "step": z[f"{tag}_{key}_step"][k].tolist(), "norm": z[f"{tag}_{key}_norm"][k]} for k in range(len(case["grads"]))]


# ---- fixtures against the restatement -----------------------------------------------------------------------------------------------
def test_schedule_restatement_is_the_reference_bitwise():
    meta, z = load_golden("optim_schedule")
    for name in ("shipped", "annealed"):
        cfg = meta[name]
        assert np.array_equal(oc.schedule(1, 12000, **cfg), z["lr_" + name]), name
        assert np.array_equal(oc.schedule(meta["restart"] + 1, meta["restart"] + len(z["restart_" + name]), **cfg), z["restart_" + name]), name
    s = z["lr_shipped"]
    assert np.argmax(s) == 3999 and s[3999] == 0.0625 * 4000 ** -0.5


def test_fixture_is_what_tiny_case_builds():
    meta, z = load_golden("optim_tiny")
    case = oc.tiny_case(0.0)
    assert [list(p.shape) for p in case["params"]] == meta["sizes"] and len(case["grads"]) == meta["steps"]
    assert np.array_equal(np.concatenate([p.reshape(-1) for p in case["params"]]), z["params"])
    for k, row in enumerate(case["grads"]):
        flat = np.concatenate([(np.full(p.shape, np.nan, np.float32) if g is None else g).reshape(-1) for g, p in zip(row, case["params"])])
        assert np.array_equal(flat, z["grads"][k], equal_nan=True), k
    for key, wd in (("wd0", 0.0), ("wd1", 0.01)):
        assert np.array_equal(np.array(oc.tiny_case(wd)["lrs"]), z["lrs_" + key])
    norms = z["ref64_wd0_norm"]
    assert norms[2] < meta["max_norm"] < norms[0], "one step below the threshold, the others above"
    assert z["ref64_wd0_step"][-1].tolist() == [5, 4, 5, 5, 5, 0], "a gradient set to None once, a never-updated tensor"


@pytest.mark.parametrize("key,name", [("wd0", "tiny"), ("wd1", "tiny_wd")])
def test_restatement_reproduces_the_reference(key, name):
    """float64 against the reference's float64 loop to round-off (1e-12 of the tensor's largest magnitude); the reference's fp32 loop
    inside the gate built from THIS torch's fp32 Adam."""
    _, z = load_golden("optim_tiny")
    case, want, t32 = oc.case(name)
    ref64, ref32 = fixture_trajectory(z, "ref64", key, case), fixture_trajectory(z, "ref32", key, case)
    for k, (w, r) in enumerate(zip(want, ref64)):
        assert w["step"] == r["step"], (k, w["step"], r["step"])
        assert abs(w["norm"] - r["norm"]) <= 1e-14 * w["norm"]
        for q in oc.QUANTITIES:
            for i, (a, b) in enumerate(zip(w[q], r[q])):
                assert np.all(np.abs(a - b) <= 1e-12 * np.max(np.abs(a)) + 1e-300), (q, k, i)
    sh = oc.worst(oc.shares(ref32, t32, want))
    print(name, "reference fp32 loop, worst share of the gate:", {q: round(v, 4) for q, v in sh.items()})
    assert all(v <= 1.0 for v in sh.values()), sh
    for k, r in enumerate(ref32):
        assert r["step"] == want[k]["step"]


@pytest.mark.parametrize("mutant", oc.MUTANTS)
def test_gate_rejects_mutant(mutant):
    name = "tiny_wd" if mutant == "decoupled_weight_decay" else "tiny"
    case, want, t32 = oc.case(name)
    sh = oc.worst(oc.shares(oc.run(case, mutate=mutant), t32, want))
    print(mutant, "worst share of the gate:", {q: round(v, 2) for q, v in sh.items()})
    assert max(sh.values()) > 1.0, (mutant, sh)


@pytest.mark.parametrize("name", list(oc.CASES))
def test_seeded_cases_are_sound(name):
    """The restatement agrees with torch's float64 Adam to round-off on every seeded case, step counts included, and the cases hold
    what their names promise."""
    case, want, t32 = oc.case(name)
    t64 = oc.torch_run(case, "float64")
    for w, r in zip(want, t64):
        assert w["step"] == r["step"]
        assert abs(w["norm"] - r["norm"]) <= 1e-13 * max(w["norm"], 1e-300)
        for q in oc.QUANTITIES:
            for a, b in zip(w[q], r[q]):
                assert a.size == 0 or np.all(np.abs(a - b) <= 1e-9 * np.max(np.abs(a)) + 1e-300), (name, q)
    assert sum(p.size for p in case["params"]) < 200_000
    norms = [w["norm"] for w in want]
    if name in ("edges", "none_comes_and_goes"):
        assert min(norms) < case["max_norm"] < max(norms)
    if name == "exact_threshold":
        assert norms == [1.0, 1.0]
    if name == "many_small":
        assert len(case["params"]) == 300 and set(p.size for p in case["params"]) == set(range(1, 8))
    if name == "edges":
        assert [p.size for p in case["params"]] == [0, 1, 3, 4, 5, oc.CHUNK - 1, oc.CHUNK, oc.CHUNK + 1, 2 * oc.CHUNK + 3]


# ---- ScheduledOptim's schedule ------------------------------------------------------------------------------------------------------
class _Holder(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.items = torch.nn.ParameterList(params)


def _train_config(schedule, weight_decay=0.0):
    return {"optimizer": dict(betas=list(oc.BETAS), eps=oc.EPS, weight_decay=weight_decay, **schedule)}


MODEL_CONFIG = {"transformer": {"encoder_hidden": oc.ENCODER_HIDDEN}}


def _schedule_only(schedule, current_step):
    """A ScheduledOptim without its device optimizer: the schedule is host arithmetic."""
    from smart_nar_fast_tts_amd.optim import ScheduledOptim

    class Groups:
        param_groups = [{"lr": None}]

    so = ScheduledOptim.__new__(ScheduledOptim)
    cfg = _train_config(schedule)["optimizer"]
    so._optimizer = Groups()
    so.n_warmup_steps, so.anneal_steps, so.anneal_rate = cfg["warm_up_step"], cfg["anneal_steps"], cfg["anneal_rate"]
    so.current_step = current_step
    so.init_lr = np.power(MODEL_CONFIG["transformer"]["encoder_hidden"], -0.5)
    return so


def test_scheduled_optim_schedule_bitwise():
    meta, z = load_golden("optim_schedule")
    for name in ("shipped", "annealed"):
        for start, want in ((0, z["lr_" + name]), (meta["restart"], z["restart_" + name])):
            so = _schedule_only(meta[name], start)
            got = []
            for _ in range(len(want)):
                so._update_learning_rate()
                got.append(so._optimizer.param_groups[0]["lr"])
            assert so.current_step == start + len(want)
            assert np.array_equal(np.array(got, dtype=np.float64), want), (name, start)
    a, s = z["lr_annealed"], z["lr_shipped"]
    assert np.array_equal(a[:3000], s[:3000]) and a[3000] != s[3000]
    for step, n in ((3001, 1), (5001, 2), (9001, 3)):
        want = np.min([np.power(step, -0.5), np.power(4000, -1.5) * step])
        for _ in range(n):
            want = want * 0.3
        assert a[step - 1] == np.power(256, -0.5) * want, step


# ---- the C ABI's host side ------------------------------------------------------------------------------------------------------------
def test_abi_version_and_constants_header_against_lib():
    from smart_nar_fast_tts_amd import optim

    lib = _lib.load()
    text = open(HEADER).read()
    assert int(re.search(r"#define NS_OPT_ABI_VERSION (\d+)", text).group(1)) == lib.ns_opt_abi_version() == 1
    assert int(re.search(r"#define NS_OPT_CHUNK (\d+)", text).group(1)) == oc.CHUNK == optim.CHUNK
    # every other ABI version stays as it is
    for macro, fn, want in (("NS_VT_ABI_VERSION", lib.ns_vt_abi_version, 1), ("NS_LOSS_ABI_VERSION", lib.ns_loss_abi_version, 1), ("NS_ABI_VERSION", lib.ns_abi_version, 6),
                            ("NS_VOC_ABI_VERSION", lib.ns_voc_abi_version, 1), ("NS_ALN_ABI_VERSION", lib.ns_aln_abi_version, 1),
                            ("NS_MEL_ABI_VERSION", lib.ns_mel_abi_version, 1), ("NS_GL_ABI_VERSION", lib.ns_gl_abi_version, 1)):
        assert int(re.search(rf"#define {macro} (\d+)", text).group(1)) == fn() == want, macro


@pytest.mark.parametrize("struct,cls,size", [("ns_opt_tensor", _lib.NsOptTensor, 40), ("ns_opt_plan", _lib.NsOptPlan, 40),
                                             ("ns_opt_record", _lib.NsOptRecord, 16), ("ns_opt_hyper", _lib.NsOptHyper, 56)])
def test_structs_match_header(struct, cls, size):
    text = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", text, flags=re.S).group(1), flags=re.S)
    fields = [f.strip().lstrip("*") for decl in re.findall(r"(?:const )?\w+\*? ([^;]+);", body) for f in decl.split(",")]
    assert fields == [f for f, _ in cls._fields_]
    assert C.sizeof(cls) == size


def _plan(sizes):
    lib = _lib.load()
    plan = _lib.NsOptPlan()
    rc = lib.ns_opt_plan_sizes((C.c_int64 * len(sizes))(*sizes), len(sizes), C.byref(plan))
    assert rc == 0, lib.ns_last_error()
    return plan


def test_planner_positive_and_monotone():
    for sizes in ([0], [0, 0, 0], [1], [5, 0, 4096]):
        p = _plan(sizes)
        assert p.n_tensors == len(sizes) and p.n_chunks >= p.n_tensors and p.table_bytes > 0 and p.ws_bytes > 0 and p.state_floats > 0
    for axis in range(3):
        prev = None
        for v in (0, 1, 3, 4, 5, 4095, 4096, 4097, 8195, 1 << 20):
            sizes = [7, 4096, 100]
            sizes[axis] = v
            p = _plan(sizes)
            cur = (p.n_chunks, p.table_bytes, p.ws_bytes, p.state_floats)
            assert prev is None or all(c >= q for c, q in zip(cur, prev)), (axis, v, cur, prev)
            prev = cur
    assert _plan([7, 4096]).table_bytes < _plan([7, 4096, 0]).table_bytes
    p = _plan([0, 1, 5, 4097])
    assert (p.n_chunks, p.table_bytes, p.ws_bytes, p.state_floats) == (5, 160, 40, 4112)


def test_table_builder_rows():
    lib = _lib.load()
    sizes = [0, 1, 5, 4097, 8192]
    n = len(sizes)
    plan = _plan(sizes)
    host = np.zeros(plan.table_bytes // 8, dtype=np.int64)
    params = (C.c_void_p * n)(0, 0x10004, 0x20000, 0x30000, 0x40000)
    grads = (C.c_void_p * n)(0x90000, 0x50000, 0, 0x60004, 0x70000)
    lags = (C.c_int32 * n)(0, 3, 0, 1, 0)
    assert lib.ns_opt_build_table((C.c_int64 * n)(*sizes), params, grads, lags, n, C.c_void_p(host.ctypes.data), host.nbytes) == 0, lib.ns_last_error()
    rows = (_lib.NsOptTensor * n).from_buffer(host)
    assert [r.chunk_begin for r in rows] == [0, 1, 2, 3, 5] and plan.n_chunks == 7
    assert [r.state_offset for r in rows] == [0, 0, 4, 12, 12 + 4100] and plan.state_floats == 12 + 4100 + 8192
    assert [r.lag for r in rows] == [0, 3, 0, 1, 0] and [r.numel for r in rows] == sizes
    assert [r.grad or 0 for r in rows] == [0, 0x50000, 0, 0x60004, 0x70000], "an empty tensor is stored as skipped"
    assert all(r.state_offset % 4 == 0 for r in rows)


def test_every_refusal_is_reached_without_a_gpu():
    lib = _lib.load()
    sizes = [0, 1, 5, 4097]
    plan = _plan(sizes)
    table, ws, rec, m, v = (C.c_void_p(a) for a in (0x1000000, 0x2000000, 0x3000000, 0x4000000, 0x5000000))  # made up, never dereferenced

    def hyper(**over):
        h = _lib.NsOptHyper()
        h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.global_step = 1e-3, 0.9, 0.98, 1e-9, 0.0, 1
        for k, val in over.items():
            setattr(h, k, val)
        return h

    good = plan

    def call(name, plan=good, table=table, table_bytes=None, ws=ws, ws_bytes=None, rec=rec, h=None, m=m, v=v, floats=None, max_norm=1.0):
        pp = C.byref(plan) if plan is not None else None
        rec = C.cast(rec, C.POINTER(_lib.NsOptRecord)) if rec is not None else None  # the header types it: ns_opt_record*
        tb = good.table_bytes if table_bytes is None else table_bytes
        if name == "ns_opt_grad_norm":
            return lib.ns_opt_grad_norm(pp, table, tb, max_norm, ws, good.ws_bytes if ws_bytes is None else ws_bytes, rec, None)
        if name == "ns_opt_scale_grads":
            return lib.ns_opt_scale_grads(pp, table, tb, rec, None)
        if name == "ns_opt_zero_grads":
            return lib.ns_opt_zero_grads(pp, table, tb, None)
        hh = h if h is not None else hyper()
        return lib.ns_opt_adam_step(pp, table, tb, C.byref(hh), m, v, good.state_floats if floats is None else floats, rec, None)

    every = ("ns_opt_grad_norm", "ns_opt_scale_grads", "ns_opt_adam_step", "ns_opt_zero_grads")

    def refused(which, match, **kw):
        for name in which:
            rc = call(name, **kw)
            msg = lib.ns_last_error().decode()
            assert rc != 0 and msg.startswith(name) and re.search(match, msg), (name, match, rc, msg)

    refused(every, "null argument", plan=None)
    refused(every, "null argument", table=None)
    refused(every, r"table too small \(ns_opt_plan_sizes\)", table_bytes=plan.table_bytes - 1)
    refused(every, "table must be 8-byte aligned", table=C.c_void_p(0x1000004))
    zero_tensors = _lib.NsOptPlan.from_buffer_copy(plan)
    zero_tensors.n_tensors = 0
    refused(every, "n_tensors must be positive", plan=zero_tensors)
    short = _lib.NsOptPlan.from_buffer_copy(plan)
    short.n_chunks = 3
    refused(every, "n_chunks is not one ns_opt_plan_sizes returns", plan=short)
    shrunk = _lib.NsOptPlan.from_buffer_copy(plan)
    shrunk.ws_bytes = 8
    refused(every, "sizes are not those ns_opt_plan_sizes returns", plan=shrunk)
    refused(("ns_opt_grad_norm",), "null argument", ws=None)
    refused(("ns_opt_grad_norm",), r"workspace too small \(ns_opt_plan_sizes\)", ws_bytes=plan.ws_bytes - 1)
    refused(("ns_opt_grad_norm",), "workspace must be 8-byte aligned", ws=C.c_void_p(0x2000004))
    refused(("ns_opt_grad_norm",), "max_norm must be >= 0", max_norm=-1.0)
    refused(("ns_opt_grad_norm",), "max_norm must be >= 0", max_norm=float("nan"))
    refused(("ns_opt_grad_norm", "ns_opt_scale_grads"), "null record", rec=None)
    refused(("ns_opt_grad_norm", "ns_opt_scale_grads"), "record must be 8-byte aligned", rec=C.c_void_p(0x3000004))
    adam = ("ns_opt_adam_step",)
    refused(adam, "null argument", m=None)
    refused(adam, "null argument", v=None)
    refused(adam, "negative size", floats=-1)
    refused(adam, r"state arena too small \(ns_opt_plan_sizes\)", floats=plan.state_floats - 1)
    refused(adam, "state arenas must be 16-byte aligned", m=C.c_void_p(0x4000008))
    refused(adam, "must be two arenas", v=m)
    for k, val in (("beta1", 1.0), ("beta1", -0.1), ("beta2", 1.0), ("beta2", float("nan"))):
        refused(adam, r"betas must lie in \[0, 1\)", h=hyper(**{k: val}))
    refused(adam, "eps must be >= 0", h=hyper(eps=-1e-9))
    refused(adam, "lr must be >= 0", h=hyper(lr=-1e-3))
    refused(adam, "weight_decay must be >= 0", h=hyper(weight_decay=-0.01))
    refused(adam, "global_step must be >= 1, got 0", h=hyper(global_step=0))
    refused(adam, "null record", h=hyper(fuse_clip=1), rec=None)
    # the host-only pair
    out = _lib.NsOptPlan()
    one = (C.c_int64 * 1)(5)
    host = np.zeros(5, dtype=np.int64)
    ptr, null = (C.c_void_p * 1)(0x10000), (C.c_void_p * 1)(0)

    def build(numels=one, params=ptr, grads=ptr, lags=None, table=host.ctypes.data, nbytes=40):
        return lib.ns_opt_build_table(numels, params, grads, lags, 1, C.c_void_p(table) if table else None, nbytes)

    for make, match in ((lambda: lib.ns_opt_plan_sizes(None, 1, C.byref(out)), "ns_opt_plan_sizes: null argument"),
                        (lambda: lib.ns_opt_plan_sizes(one, 1, None), "ns_opt_plan_sizes: null argument"),
                        (lambda: lib.ns_opt_plan_sizes(one, 0, C.byref(out)), "n_tensors must be positive, got 0"),
                        (lambda: lib.ns_opt_plan_sizes((C.c_int64 * 1)(-1), 1, C.byref(out)), "negative size of tensor 0"),
                        (lambda: lib.ns_opt_plan_sizes((C.c_int64 * 1)(1 << 41), 1, C.byref(out)), "problem too large"),
                        (lambda: build(params=None), "ns_opt_build_table: null argument"),
                        (lambda: build(table=0), "ns_opt_build_table: null argument"),
                        (lambda: build(nbytes=39), "table too small"),
                        (lambda: build(table=host.ctypes.data + 4), "table must be 8-byte aligned"),
                        (lambda: build(params=null), "null parameter pointer of tensor 0"),
                        (lambda: build(grads=(C.c_void_p * 1)(0x10002)), "must be 4-byte aligned"),
                        (lambda: build(lags=(C.c_int32 * 1)(-1)), "negative lag of tensor 0")):
        rc = make()
        msg = lib.ns_last_error().decode()
        assert rc != 0 and match in msg, (match, rc, msg)
    assert build() == 0


def test_header_is_plain_c_and_validation_works_from_c(tmp_path):
    run_c_caller("opt_host_only", _lib.LIB_PATH, tmp_path)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def test_python_refusals_without_a_gpu():
    import smart_nar_fast_tts_amd as pkg
    from smart_nar_fast_tts_amd import optim

    assert pkg.ScheduledOptim is optim.ScheduledOptim
    w = torch.nn.Parameter(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="must live on the MI355X .* no CPU path"):
        optim.Adam([w])
    with pytest.raises(RuntimeError, match="no CPU path"):
        optim.clip_grad_norm_([w], 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        optim.ScheduledOptim(_Holder([w]), _train_config(oc.SHIPPED), MODEL_CONFIG, 0)
    with pytest.raises(ValueError, match="parameter 0 must be float32, got torch.float64"):
        optim.Adam([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError, match="parameter 1 must be contiguous"):
        optim.Adam([w, torch.nn.Parameter(torch.zeros(4, 3).t())])
    with pytest.raises(ValueError, match="one parameter group is supported, got 2"):
        optim.Adam([{"params": [w]}, {"params": [torch.nn.Parameter(torch.zeros(2))]}])
    with pytest.raises(ValueError, match="empty parameter list"):
        optim.Adam([])
    with pytest.raises(ValueError, match="amsgrad and maximize are out of scope"):
        optim.Adam([w], amsgrad=True)
    with pytest.raises(ValueError, match="Invalid beta parameters"):
        optim.Adam([w], betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="Invalid epsilon value"):
        optim.Adam([w], eps=-1.0)
    with pytest.raises(ValueError, match="Invalid learning rate"):
        optim.Adam([w], lr=-1.0)
    with pytest.raises(ValueError, match="only the 2-norm"):
        optim.clip_grad_norm_([w], 1.0, norm_type=1.0)
    # what stays refused elsewhere
    from smart_nar_fast_tts_amd.loss import FastSpeech2Loss
    import smart_nar_fast_tts_amd.workload as wl

    with pytest.raises(NotImplementedError, match="training is out of scope"):
        FastSpeech2Loss(wl.preprocess_config(), wl.model_config("tiny")).train()


def test_optim_kernels_do_not_spill():
    assert_no_spill("optim.hip", kernels=("k_opt_sumsq", "k_opt_norm_final", "k_opt_scale", "k_opt_adam", "k_opt_zero"))
