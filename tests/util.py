"""Shared test support: fixture loading and weight rebuild, the native library for a test module, the plain-C caller and the no-spill
run, the report line, and the project's gate (DESIGN.md "Shared test and bench support").  torch is imported inside the functions that
need it, so the numpy-only yardsticks can import this module."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return meta, z


# ---- the native library, the device ---------------------------------------------------------------------------------------------------
def native_lib():
    """(smart_nar_fast_tts_amd._lib, the loaded shared library): what a module's ``so`` fixture returns"""
    import smart_nar_fast_tts_amd._lib as L

    return L, L.load()


def built_lib():
    """native_lib() after __graft_entry__.build(): what a host test module's ``lib`` fixture returns"""
    import __graft_entry__ as ge

    ge.build()
    return native_lib()


def dev(a):
    """a numpy array as a contiguous tensor on the GPU"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- subprocess checks of the host tests --------------------------------------------------------------------------------------------
def run_c_caller(stem, lib_path, tmp_path):
    """Compile tests/cabi/<stem>.c as strict C99 against include/ and run it on the library; returns what it printed.  (No copy this
    replaced passed further compiler arguments.)"""
    exe = tmp_path / stem
    src = os.path.join(ROOT, "tests", "cabi", stem + ".c")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", str(exe), "-ldl"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([str(exe), lib_path], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "C caller ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    return r.stdout


def assert_no_spill(*hip_files, kernels=(), timeout=900):
    """tools/kernel_resources.py --assert-no-spill on each of csrc/<file>; every name of ``kernels`` must be in the tables.  Returns
    the tables (stdout of all files) for the caller's further assertions."""
    out = ""
    for src in hip_files:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), os.path.join(ROOT, "smart-nar_fast_tts_amd", "csrc", src),
                            "--assert-no-spill"], capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, r.stdout + r.stderr
        out += r.stdout
    for k in kernels:
        assert k in out, (k, out)
    return out


def expect_refusals(err, call, table):
    """every (kwargs, message) of ``table``: ``call(**kwargs)`` is refused and ``err()`` holds the message"""
    for kw, msg in table:
        assert call(**kw) != 0 and msg in err(), (call.__name__, kw, err())


def reporter(env):
    """report(**row): print one JSON line and append it to the file the environment variable ``env`` names"""
    def report(**row):
        print(json.dumps(row))
        path = os.environ.get(env)
        if path:
            with open(path, "a") as f:
                f.write(json.dumps(row) + "\n")

    return report


report = reporter("NS_FP32_OPS_REPORT")  # tools/*_bench.py --report read these lines; four older test files keep a variable of their own


# ---- the gate ---------------------------------------------------------------------------------------------------------------------------
def ulp32(x):
    """one fp32 ulp at the scalar |x|; ulp32(0) is the smallest denormal"""
    return float(np.spacing(np.float32(abs(float(x)))))


def gate_value(ref32, ref64):
    """The project's absolute gate of one tensor, the one written-out copy: twice the reference's own fp32 error plus one fp32 ulp of
    the largest float64 magnitude.  An all-zero (or empty) float64 tensor has a gate of one denormal: it must be matched exactly."""
    a, b = np.asarray(ref32, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    return 2.0 * float(np.max(np.abs(a - b), initial=0.0)) + ulp32(np.max(np.abs(b), initial=0.0))


def gates(ref32, ref64, names=None):
    """{name: gate_value}; ``names`` defaults to the keys of ref64 that ref32 also has"""
    return {n: gate_value(ref32[n], ref64[n]) for n in (names or [n for n in ref64 if n in ref32])}


def share_of(got, want64, gate):
    """(max |got - want64| / gate, flat index of the worst element) of one tensor; a NaN or Inf anywhere in ``got`` gives inf at the
    first such element, an empty tensor (0.0, -1)"""
    a, w = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    if a.size == 0:
        return 0.0, -1
    if not np.isfinite(a).all():
        return float("inf"), int(np.argmax(~np.isfinite(a)))
    err = np.abs(a - w)
    return float(err.max() / gate), int(err.argmax())


def shares(got, ref64, gates, names=None):
    """{name: max |got - ref64| / gate} over ``names`` (default: the gates' keys), got[name] taken in ref64[name]'s shape; inf for a
    NaN / Inf in got.  A missing (None) entry is skipped."""
    return {n: share_of(np.asarray(got[n]).reshape(np.asarray(ref64[n]).shape), ref64[n], gates[n])[0]
            for n in (names or gates) if got.get(n) is not None}


_SD_CACHE = {}


def weights_for(meta):
    """Rebuild the seeded weights a fixture was generated with (they are not stored)."""
    import smart_nar_fast_tts_amd.workload as wl

    key = (meta["config"], meta.get("weight_seed", 0), meta["frames_per_phoneme"], meta.get("dur_weight_scale", 0.25))
    if key not in _SD_CACHE:
        cfg = wl.model_config(meta["config"])
        _SD_CACHE.clear()  # one at a time: a full state dict is 116 MB
        _SD_CACHE[key] = (cfg, wl.synth_state_dict(cfg, seed=key[1], frames_per_phoneme=key[2], dur_weight_scale=key[3]))
    return _SD_CACHE[key]


F64_FIXTURES = {"f64_cfg1": "pin_cfg1_single", "f64_cfg2": "pin_cfg2_b16", "f64_cfg4": "pin_cfg4_d512", "f64_cfg5": "pin_cfg5_longform"}


def _dist_stats(d):
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    if d.size == 0:
        return {"max": 0.0, "p999": 0.0, "median": 0.0, "n": 0}
    return {"max": float(d.max()), "p999": float(np.quantile(d, 0.999)), "median": float(np.median(d)), "n": int(d.size)}


def accuracy_against_float64(name, model, sd):
    """|HIP - float64| beside |reference-fp32 - float64| on one float64 fixture (tests/golden/f64_cfg*.npz, written by
    tools/reference_self_deviation.py from the imported reference cast to .double(), bucket decisions pinned to the fp32
    reference's own predictions).  The HIP forward takes the SAME decisions (p_targets / e_targets = the fp32 pin's predictions),
    so all three evaluations compute the same function and differ in arithmetic only.

    Returns ``{quantity: {"hip": stats, "ref32": stats}}`` with stats = max / p99.9 / median; pitch and energy relative to
    max(|truth|, 1) on the frames inside the bin range (oracle/parity.py), log-duration and the two mels absolute, mels on every
    ``frame_stride``-th frame (what the fixture holds)."""
    import torch

    from oracle import parity

    meta64, z64 = load_golden(name)
    meta, z = load_golden(meta64["source_pin"])
    stride = int(meta64["frame_stride"])
    with torch.no_grad():
        out = model(dev(z["speakers"]), dev(z["texts"]), dev(z["in_src_lens"]), int(meta["L"]),
                    p_targets=dev(z["p_predictions"]), e_targets=dev(z["e_predictions"]))
    torch.cuda.synchronize()
    assert np.array_equal(out[9].cpu().numpy(), z["mel_lens"]), (name, "frame counts differ from the reference's")
    assert np.array_equal(out[5].cpu().numpy(), z["d_rounded"]), (name, "durations differ from the reference's")
    valid = ~z["mel_masks"]
    src_valid = np.arange(z["log_d_predictions"].shape[1])[None, :] < z["in_src_lens"][:, None]
    vs = valid[:, ::stride]
    res = {}

    def both(key, hip, ref32, truth, sel, rel):
        t = np.asarray(truth, dtype=np.float64)
        den = np.maximum(np.abs(t), 1.0) if rel else 1.0
        res[key] = {"hip": _dist_stats((np.abs(np.asarray(hip, dtype=np.float64) - t) / den)[sel]),
                    "ref32": _dist_stats((np.abs(np.asarray(ref32, dtype=np.float64) - t) / den)[sel])}

    both("log_d", out[4].cpu().numpy(), z["log_d_predictions"], z64["log_d_predictions"], src_valid, False)
    for key, i, k, bins in (("pitch_rel", 2, "p_predictions", "variance_adaptor.pitch_bins"), ("energy_rel", 3, "e_predictions", "variance_adaptor.energy_bins")):
        both(key, out[i].cpu().numpy(), z[k], z64[k], parity.in_range(z[k], np.asarray(sd[bins]), valid), True)
    both("mel", out[0].cpu().numpy()[:, ::stride], z["output_sub"], z64["output_sub"], vs, False)
    both("postnet", out[1].cpu().numpy()[:, ::stride], z["postnet_output_sub"], z64["postnet_output_sub"], vs, False)
    return res
