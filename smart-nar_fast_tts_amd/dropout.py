"""Dropout keep-masks from a counter-based generator in HIP (csrc/keepmask.hip through ``ns_km_*``).

    rng = dropout.KeepMaskRNG(seed=1234)
    dropout.attach(model, rng)                 # every trainable HIP layer below ``model`` now draws from ``rng``
    losses = training.train_step(model, Loss, optimizer, batch, step, 1, 1.0)     # all 40 masks of the step: ONE launch
    training.save_checkpoint(model, optimizer, path, rng=rng)
    ...
    rng.load_state_dict(torch.load(path, weights_only=True)["keep_mask_rng"])      # the resumed run draws what the first would have

A mask's bytes are a pure function of ``(seed, call, stream, element index)`` — Philox4x32-10 at counter ``(element >> 2, stream, call)``
under the key ``seed``, kept where the element's word is below ``floor((1 - p) * 2^32)`` (include/nar_fs2.h states the rule) — so a mask
does not depend on which other masks are drawn with it: a whole step's masks drawn into one arena (``prefetch``) and the same masks
drawn module by module (``take``) are the same bits.  With no generator attached every layer draws with ``torch.bernoulli`` as before."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._train import HipTrainModule, guard

_ROW = np.dtype([("offset", "<u8"), ("n", "<u8"), ("stream", "<u4"), ("thr", "<u4"), ("chunk_begin", "<u8")])  # csrc/keepmask.h KmEntry
assert _ROW.itemsize == _lib.KM_TABLE_ROW_BYTES


def threshold(p) -> int:
    """``ns_km_threshold``: ``floor((1.0 - p) * 2^32)`` in float64; raises for ``p`` outside (0, 1) or a threshold of 0."""
    thr = C.c_uint32(0)
    _lib.check(_lib.load().ns_km_threshold(float(p), C.byref(thr)), "ns_km_threshold")
    return thr.value


def _device(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("KeepMaskRNG: the masks are drawn on the MI355X (there is no CPU path)")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def _entries(shapes, p):
    return tuple((tuple(int(d) for d in s), float(p)) for s in shapes)


class KeepMaskRNG:
    """The generator's state is three integers: ``seed`` (64 bits), ``call`` (the draw counter, 64 bits) and ``stream`` (the id the next
    mask of this call gets, 32 bits).

    ``next_call()`` increments ``call`` and sets ``stream`` to 0: one per training step (``training.FastSpeech2Align.forward`` makes it).
    ``take(shapes, p, device)`` returns one uint8 tensor (1 = kept) per shape, each 16-byte aligned, and consumes ``len(shapes)``
    consecutive stream ids: views of the prefetched arena when one is active and its next planned entries are these ``(shape, p)`` (a
    mismatch raises, naming both), else one ``ns_km_draw`` of just these masks.
    ``prefetch(entries, device)`` draws a whole list of ``(shape, p)`` — the masks the coming ``take`` calls will ask for, in their
    order — in one ``ns_km_draw`` into a fresh arena from torch's allocator (the views handed out keep it alive until the backward
    has run).  The device table of a list is cached per ``(device, first stream, entries)``; its upload is a host-to-device copy.
    ``launches`` counts the draws.  ``state_dict()`` is plain Python ints, so ``torch.load(..., weights_only=True)`` takes it."""

    VERSION = 1
    MAX_TABLES = 16

    def __init__(self, seed):
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must lie in [0, 2^64), got {seed}")
        self.seed, self.call, self.stream = seed, 0, 0
        self.launches = 0
        self._lib = _lib.load()
        self._tables = OrderedDict()
        self._planned, self._cursor = [], 0  # the active prefetch: [(shape, p, view)] and how many were handed out

    # ---- state
    def state_dict(self):
        return {"version": self.VERSION, "seed": self.seed, "call": self.call, "stream": self.stream}

    def load_state_dict(self, state):
        if state.get("version") != self.VERSION:
            raise ValueError(f"keep_mask_rng state has version {state.get('version')!r}, this KeepMaskRNG reads version {self.VERSION}")
        seed, call, stream = int(state["seed"]), int(state["call"]), int(state["stream"])
        if not (0 <= seed < 1 << 64 and 0 <= call < 1 << 64 and 0 <= stream < 1 << 32):
            raise ValueError(f"keep_mask_rng state out of range: seed {seed}, call {call}, stream {stream}")
        self.seed, self.call, self.stream = seed, call, stream
        self._planned, self._cursor = [], 0

    def next_call(self):
        self.call = (self.call + 1) & ((1 << 64) - 1)
        self.stream = 0
        self._planned, self._cursor = [], 0

    # ---- draws
    def _table(self, entries, device):
        """(device table, arena bytes, byte offsets) of ``entries`` at the current stream"""
        key = (device.index, torch.cuda.current_stream(device).cuda_stream, self.stream, entries)  # (the upload is ordered on that stream)
        hit = self._tables.get(key)
        if hit is None:
            n = len(entries)
            if self.stream + n > 1 << 32:
                raise ValueError(f"stream ids are 32 bits: {self.stream} + {n} masks in one call")
            masks = (_lib.NsKmMask * max(n, 1))()
            for i, (shape, p) in enumerate(entries):
                if len(shape) == 0 or min(shape) <= 0:
                    raise ValueError(f"a keep-mask must not be empty, got shape {shape}")
                masks[i].n, masks[i].stream, masks[i].thr = int(np.prod(shape, dtype=np.int64)), self.stream + i, threshold(p)
            nbytes = self._lib.ns_km_table_bytes(n)
            if nbytes == 0:
                _lib.check(1, "ns_km_table_bytes")
            host = np.zeros(nbytes, dtype=np.uint8)
            arena_bytes = C.c_uint64(0)
            _lib.check(self._lib.ns_km_plan(masks, n, host.ctypes.data, nbytes, C.byref(arena_bytes)), "ns_km_plan")
            offsets = tuple(int(o) for o in host.view(_ROW)["offset"][:n])
            # the upload: one host-to-device copy from pinned memory, in stream order (no synchronisation); the pinned copy stays with
            # the cache entry, so it outlives the transfer
            pinned = torch.from_numpy(host).pin_memory()
            hit = (pinned.to(device, non_blocking=True), int(arena_bytes.value), offsets, pinned)
            self._tables[key] = hit
        self._tables.move_to_end(key)
        while len(self._tables) > self.MAX_TABLES:
            self._tables.popitem(last=False)
        return hit

    def _draw(self, entries, device):
        """one ``ns_km_draw`` of ``entries`` at the streams [stream, stream + len): the masks as views of a fresh arena"""
        with guard(device):
            table, arena_bytes, offsets = self._table(entries, device)[:3]
            arena = torch.empty(arena_bytes, dtype=torch.uint8, device=device)
            _lib.check(self._lib.ns_km_draw(_lib.ptr(table), len(entries), self.seed, self.call, _lib.ptr(arena), arena_bytes, _lib.stream_ptr(device)),
                       "ns_km_draw")
        self.launches += self._lib.ns_km_last_launches()
        return [arena[o:o + int(np.prod(s, dtype=np.int64))].view(s) for o, (s, _) in zip(offsets, entries)]

    def prefetch(self, entries, device):
        """One ``ns_km_draw`` of every ``(shape, p)`` of ``entries`` at the streams the coming ``take`` calls will consume."""
        entries = tuple((tuple(int(d) for d in s), float(p)) for s, p in entries)
        self._planned, self._cursor = [], 0
        if not entries:
            return
        views = self._draw(entries, _device(device))
        self._planned = [(s, p, v) for (s, p), v in zip(entries, views)]

    def take(self, shapes, p, device):
        want, device = _entries(shapes, p), _device(device)
        left = self._planned[self._cursor:]
        if left:
            have = tuple((s, q) for s, q, _ in left[:len(want)])
            if have != want or device != left[0][2].device:
                raise RuntimeError(f"KeepMaskRNG.take: asked for {want} on {device}, but the prefetched arena has {have} on {left[0][2].device} next "
                                   f"(entry {self._cursor} of {len(self._planned)}): prefetch the masks in the order the forward consumes them")
            out = tuple(v for _, _, v in left[:len(want)])
            self._cursor += len(want)
        else:
            out = tuple(self._draw(want, device))
        self.stream += len(want)
        return out


def attach(module, rng):
    """Sets ``rng`` (a ``KeepMaskRNG``) on every trainable HIP layer at or below ``module`` — and on a ``training.FastSpeech2Align``,
    which then prefetches a step's masks in one launch.  A layer with a generator draws its masks from it whenever it would have
    drawn them with ``torch.bernoulli``; given ``keep_masks=`` still win."""
    if rng is not None and not isinstance(rng, KeepMaskRNG):
        raise TypeError(f"rng must be a dropout.KeepMaskRNG, got {type(rng).__name__}")
    n = 0
    for m in module.modules():
        if isinstance(m, HipTrainModule) or getattr(type(m), "TAKES_KEEP_MASK_RNG", False):
            m._keep_mask_rng = rng
            n += 1
    if n == 0:
        raise ValueError(f"{type(module).__name__} has no trainable HIP layer to attach a generator to")
    return module


def detach(module):
    """Removes the generator: every layer below ``module`` draws with ``torch.bernoulli`` again."""
    return attach(module, None)
