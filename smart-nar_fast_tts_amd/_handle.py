"""The Python side of ``csrc/host_core.h``: what the wrappers of the five C-ABI handle families (``ns``, ``ns_aln``, ``ns_voc``,
``ns_mel``, ``ns_gl``; include/nar_fs2.h) share.

``NativeHandle``      one native handle and its life cycle: create, check_weight, bind_arena, set_weight, finalize_weights, destroy
``StreamWorkspaces``  one LRU cache of per-stream scratch tensors; the key, the growth rule and the bound are its arguments
``DeviceModule``      the nn.Module-shaped surface (eval / train / to / cuda) of a class that owns one handle, one arena and one cache
``host_f32``          what every ``load_state_dict`` does to an entry before the library sees it

LEFT APART on purpose: ``model.FastSpeech2Align``'s own scratch cache (``_workspace``, ``_evict_streams``, ``_pinned_lens``,
``_device_lens``, ``_ws_bytes``).  It sits on the forward's hot path that bench.py times, is keyed by (kind, stream), holds entries
that are no tensors (a pinned buffer with its numpy view) and evicts whole streams, not entries.  ``_train.WorkspaceCache`` is keyed
by shape and is a different thing again.  ``FastSpeech2Align`` also keeps its own ``to()``: two handles, adopted arenas."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib


def host_f32(t) -> np.ndarray:
    """A tensor or anything array-like as a contiguous float32 numpy array on the host."""
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32)


def cuda_device(device, what: str) -> torch.device:
    """``device`` as a ``cuda:N`` torch.device with its index filled in; anything else has no path here."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"this {what} runs on an MI355X only (device must be 'cuda[:N]'); there is no CPU path")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _dims(a: np.ndarray):
    return (C.c_int64 * a.ndim)(*a.shape)


class NativeHandle:
    """``{prefix}_create(config)`` and everything host_core.h gives the handle it returns.  An instance passes as the handle
    argument of any C entry point (``_as_parameter_``) and is truthy until ``close()``.  ``what`` labels, as everywhere, the
    RuntimeError a failing call raises (``_lib.check``)."""

    def __init__(self, prefix: str, config, what: str):
        lib = _lib.load()
        self.prefix = prefix
        # symbols resolved once, here, not by name per call
        for op in ("destroy", "arena_bytes", "bind_arena", "set_weight", "check_weight", "finalize_weights"):
            setattr(self, "_" + op, getattr(lib, f"{prefix}_{op}"))
        self._last_error = lib.ns_last_error
        h = C.c_void_p()
        _lib.check(getattr(lib, f"{prefix}_create")(C.byref(config), C.byref(h)), what)
        self._as_parameter_ = h

    def __bool__(self):
        return bool(self._as_parameter_)

    def close(self):
        """Destroy the native handle; harmless when repeated, and during interpreter shutdown."""
        try:
            if getattr(self, "_as_parameter_", None):
                h, self._as_parameter_ = self._as_parameter_, C.c_void_p()
                self._destroy(h)
        except Exception:
            pass

    __del__ = close

    def check_weight(self, key: str, a: np.ndarray) -> str:
        """'' when the library accepts this key name and shape, else its error text.  No side effect on the handle."""
        if self._check_weight(self, key.encode(), _dims(a), a.ndim) == 0:
            return ""
        return self._last_error().decode()

    def set_weight(self, key: str, a: np.ndarray, what: str):
        """Hand one (already validated) contiguous float32 array to the native staging area."""
        _lib.check(self._set_weight(self, key.encode(), C.c_void_p(a.ctypes.data), _dims(a), a.ndim), what)

    def bind_arena(self, device) -> torch.Tensor:
        """A fresh arena on ``device``, bound: the handle stops pointing at whatever it was bound to before."""
        nbytes = self._arena_bytes(self)
        with torch.cuda.device(device):
            arena = torch.empty(nbytes, dtype=torch.uint8, device=device)
            _lib.check(self._bind_arena(self, _lib.ptr(arena), nbytes), f"{self.prefix}_bind_arena")
        return arena

    def finalize(self, device, what: str):
        """Pack what was staged into the bound arena, on the current stream of ``device`` (the caller has made it current)."""
        _lib.check(self._finalize_weights(self, _lib.stream_ptr(device)), what)

    def upload(self, device, weights, what: str) -> torch.Tensor:
        """bind_arena, set_weight for every entry of ``weights``, finalize; returns the new arena."""
        arena = self.bind_arena(device)
        with torch.cuda.device(device):
            for k, a in weights.items():
                self.set_weight(k, a, what)
            self.finalize(device, what)
        return arena


class StreamWorkspaces(OrderedDict):
    """Scratch tensors, one per HIP stream (calls on different streams may overlap on the GPU and must not share temporaries),
    least recently used first, at most ``max_streams`` of them: a dropped one goes back to torch's caching allocator.
    ``per_device``: keyed by (device index, stream handle) instead of the stream handle alone, for an owner that is not tied to one
    device.  ``slack``: a buffer that has to grow is sized ``1.25 n + 256`` bytes instead of exactly ``n``."""

    def __init__(self, max_streams: int, per_device: bool = False, slack: bool = False):
        super().__init__()
        self.max_streams, self.per_device, self.slack = max_streams, per_device, slack

    def take(self, device, nbytes: int, stream_handle=None) -> torch.Tensor:
        """The buffer of ``stream_handle`` (default: the current stream of ``device``), at least ``nbytes`` long."""
        if stream_handle is None:
            stream_handle = torch.cuda.current_stream(device).cuda_stream
        key = (device.index, stream_handle) if self.per_device else stream_handle
        w = self.get(key)
        if w is None or w.numel() < nbytes:
            w = torch.empty(int(nbytes * 1.25) + 256 if self.slack else int(nbytes), dtype=torch.uint8, device=device)
            self[key] = w
        self.move_to_end(key)
        while len(self) > self.max_streams:
            self.popitem(last=False)
        return w


class DeviceModule:
    """The nn.Module-shaped part of a class that owns one native handle: eval / train / to / cuda, the arena and one workspace per
    HIP stream.  A subclass calls ``_open()`` in its constructor, ends its ``load_state_dict`` with ``_loaded(new)`` and may override
    ``_weights()``.

    Threading: one instance serves one host thread at a time; several HIP streams from that thread are fine (one workspace each)."""

    MAX_WORKSPACE_STREAMS = 4
    KIND = "front end"                                       # "this ... runs on an MI355X only"
    NO_TRAINING = "the front end has no trainable state"
    PICKS_DEVICE_ON_LOAD = False                             # load_state_dict on a module nobody moved: upload to the current device

    def _open(self, prefix: str, config, what: str):
        self._lib = _lib.load()
        self._h = NativeHandle(prefix, config, what)
        self._device = None
        self._arena = None
        self._sd = None  # key -> host float32 array, what load_state_dict accepted
        self._ws = StreamWorkspaces(self.MAX_WORKSPACE_STREAMS)
        self.training = False

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None:
            h.close()

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError(self.NO_TRAINING)
        return self.eval()

    def to(self, device):
        device = cuda_device(device, self.KIND)
        if self._device != device:
            self._device = device
            self._ws.clear()
            self._arena = None
            if self._sd is not None:
                self._upload()  # (binds a fresh arena first: the handle never keeps the old device's)
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def state_dict(self):
        return OrderedDict((k, torch.from_numpy(v.copy())) for k, v in (self._sd or {}).items())

    def _weights(self):
        """key -> array as the library names them."""
        return self._sd

    def _upload(self):
        self._arena = self._h.upload(self._device, self._weights(), "load_state_dict")

    def _loaded(self, new):
        """The tail of a ``load_state_dict`` that found nothing to refuse: keep ``new``, upload if there is a device."""
        self._sd = new
        if self.PICKS_DEVICE_ON_LOAD and self._device is None and torch.cuda.is_available():
            self._device = torch.device("cuda", torch.cuda.current_device())
        if self._device is not None:
            self._upload()
        return [], []

    def release_workspaces(self):
        self._ws.clear()
