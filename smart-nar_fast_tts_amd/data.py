"""A device-resident training set (csrc/dataset.hip through ``ns_ds_*``): the reference's ``Dataset`` +
``DataLoader`` + ``to_device`` (dataset.py:12-139, train.py:27-38 and 75-77, utils/tools.py:18-54) with the set uploaded ONCE and every
batch made by ONE gather launch.

    train_set = data.DeviceDataset.from_preprocessed("train.txt", preprocess_config, train_config, text_to_sequence, device)
    for batch in train_set.epoch(batch_size):                       # the reference's 11-tuple, tensors on the device
        losses = training.train_step(model, Loss, optimizer, batch, step, grad_acc_step, grad_clip_thresh)

The packed store (mel [sum T, n_mel] fp32, pitch / energy fp32 and text int32 as ragged 1-D arrays with 16-byte slots, speaker int32,
the offset tables and the length vectors) is read-only after the upload.  ``epoch()`` plans the epoch's batches on the host from the
text lengths (``plan_epoch``: pure numpy, the reference's grouping and ``np.argsort(-len_arr)``), uploads the epoch's order once, and
then per batch allocates the seven outputs with ``torch.empty`` and calls ``ns_ds_gather``: one launch, no memset, no host read.
There is no CPU path: a store on a device other than the GPU raises."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import torch

from . import _lib
from ._train import guard

NsDsLens, NsDsOffsets, NsDsStore, NsDsBatch = (_lib.STRUCTS[n] for n in ("ns_ds_lens", "ns_ds_offsets", "ns_ds_store", "ns_ds_batch"))
LEVELS = ("phoneme_level", "frame_level")


def plan_epoch(text_lens, batch_size, group_size=4, sort=True, drop_last=True, perm=None, generator=None):
    """The index batches (a list of int64 arrays) of one epoch as the reference's loader yields them: ``perm`` (default
    ``torch.randperm(n, generator=generator)``, what ``DataLoader(shuffle=True)``'s sampler draws) cut into consecutive groups of
    ``batch_size * group_size`` (train.py:30-38), the last one partial; every group sorted with ``np.argsort(-len_arr)`` when ``sort``
    (dataset.py:123-125: numpy's default kind, so ties fall as numpy lets them), cut into batches, and its partial tail dropped when
    ``drop_last`` (dataset.py:129-133).  Pure numpy: no device.  Validation is ``sort=False, drop_last=False, group_size=1,
    perm=np.arange(n)``."""
    text_lens = np.asarray(text_lens)
    n = int(text_lens.shape[0])
    batch_size, group_size = int(batch_size), int(group_size)
    if text_lens.ndim != 1 or batch_size < 1 or group_size < 1:
        raise ValueError(f"plan_epoch: text_lens must be a vector and batch_size, group_size positive, got {text_lens.shape}, {batch_size}, {group_size}")
    perm = torch.randperm(n, generator=generator).numpy() if perm is None else np.asarray(perm, dtype=np.int64)
    if perm.ndim != 1 or (perm.size and (perm.min() < 0 or perm.max() >= n)):
        raise ValueError(f"plan_epoch: perm must hold indices in [0, {n})")
    batches = []
    for g0 in range(0, perm.size, batch_size * group_size):
        group = perm[g0:g0 + batch_size * group_size]
        if sort:
            len_arr = np.array([int(v) for v in text_lens[group]])
            idx_arr = np.argsort(-len_arr)
        else:
            idx_arr = np.arange(group.size)
        tail = idx_arr[len(idx_arr) - (len(idx_arr) % batch_size):]
        idx_arr = idx_arr[:len(idx_arr) - (len(idx_arr) % batch_size)]
        batches += [group[row].astype(np.int64) for row in idx_arr.reshape((-1, batch_size))]
        if not drop_last and len(tail) > 0:
            batches.append(group[tail].astype(np.int64))
    return batches


def _level(preprocess_config, what):
    level = preprocess_config["preprocessing"][what]["feature"]
    if level not in LEVELS:
        raise ValueError(f"preprocessing.{what}.feature must be one of {LEVELS}, got {level!r}")
    return level


class DeviceDataset:
    """The whole preprocessed set on the GPU.  ``len()`` utterances; ``ids`` / ``raw_texts`` (host lists), ``text_lens`` / ``mel_lens`` /
    ``pitch_lens`` / ``energy_lens`` (host int32 vectors: all the host keeps), ``skipped`` (the ids ``max_frames`` left out),
    ``upload_bytes``; ``launches`` / ``last_launches`` count the gather launches as the C side counted them."""

    def __init__(self):
        raise TypeError("build a DeviceDataset with from_arrays() or from_preprocessed()")

    # ---- construction
    @classmethod
    def from_arrays(cls, ids, raw_texts, speakers, texts, mels, pitches, energies, preprocess_config, device, max_frames=None):
        """``ids`` / ``raw_texts``: lists of N strings; ``speakers``: N speaker ids; ``texts``: N integer vectors [L_i]; ``mels``: N arrays
        [T_i, n_mel]; ``pitches`` / ``energies``: N vectors of T_i (``frame_level``) or L_i (``phoneme_level``) values, as
        ``preprocess_config`` says.  Everything is converted to fp32 / int32, packed and uploaded: one upload per array.  Raises
        ``ValueError`` naming the utterance for a pitch or energy length its feature level does not give, and for an ``n_mel`` other
        than the config's.  ``max_frames`` (an extension) leaves out the utterances longer than that many frames and lists their ids
        in ``.skipped`` (``training.FastSpeech2Align`` refuses a mel longer than ``max_seq_len`` in ``train()``)."""
        n_mel = int(preprocess_config["preprocessing"]["mel"]["n_mel_channels"])
        levels = (_level(preprocess_config, "pitch"), _level(preprocess_config, "energy"))
        n = len(ids)
        if not (len(raw_texts) == len(speakers) == len(texts) == len(mels) == len(pitches) == len(energies) == n):
            raise ValueError("from_arrays: ids, raw_texts, speakers, texts, mels, pitches and energies must have one length")
        keep, skipped = [], []
        for i in range(n):
            mel, text = np.asarray(mels[i]), np.asarray(texts[i])
            if mel.ndim != 2 or mel.shape[1] != n_mel:
                raise ValueError(f"utterance {ids[i]!r}: the mel must be [T, n_mel = {n_mel}] (preprocessing.mel.n_mel_channels), got {mel.shape}")
            if text.ndim != 1 or text.shape[0] < 1 or mel.shape[0] < 1:
                raise ValueError(f"utterance {ids[i]!r}: the text must be a vector of at least one phoneme and the mel at least one frame, got "
                                 f"{text.shape} and {mel.shape}")
            for what, level, a in (("pitch", levels[0], pitches[i]), ("energy", levels[1], energies[i])):
                want = mel.shape[0] if level == "frame_level" else text.shape[0]
                if np.ndim(a) != 1 or len(a) != want:
                    raise ValueError(f"utterance {ids[i]!r}: {what} is {level}, so it must hold {want} values ({'T' if level == 'frame_level' else 'L'}), "
                                     f"got shape {np.shape(a)}")
            if max_frames is not None and mel.shape[0] > int(max_frames):
                skipped.append(ids[i])
            else:
                keep.append(i)
        if not keep:
            raise ValueError("from_arrays: no utterance left")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("DeviceDataset: the set lives on the MI355X (there is no CPU path)")
        device = torch.device("cuda", torch.cuda.current_device()) if device.index is None else device

        self = object.__new__(cls)
        self._lib = _lib.load()
        self.device, self.n_mel, self.skipped = device, n_mel, skipped
        self.ids, self.raw_texts = [ids[i] for i in keep], [raw_texts[i] for i in keep]
        N = len(keep)
        lens = [np.array([len(src[i]) for i in keep], dtype=np.int32) for src in (texts, mels, pitches, energies)]
        self.text_lens, self.mel_lens, self.pitch_lens, self.energy_lens = lens
        self._host_lens = NsDsLens(*(a.ctypes.data for a in lens))
        off = np.zeros((4, N + 1), dtype=np.int64)  # mel, pitch, energy, text
        nbytes = (C.c_uint64 * 4)()
        _lib.check(self._lib.ns_ds_plan(C.byref(self._host_lens), N, n_mel, C.byref(NsDsOffsets(*(off[k].ctypes.data for k in range(4)))), nbytes),
                   "ns_ds_plan")
        mel = np.empty((int(off[0, N]), n_mel), dtype=np.float32)
        flat = [np.zeros(int(off[k, N]), dtype=dt) for k, dt in ((1, np.float32), (2, np.float32), (3, np.int32))]
        assert [mel.nbytes] + [a.nbytes for a in flat] == [int(b) for b in nbytes]
        for j, i in enumerate(keep):
            mel[off[0, j]:off[0, j + 1]] = np.asarray(mels[i], dtype=np.float32)
            for k, src in ((1, pitches), (2, energies), (3, texts)):
                flat[k - 1][off[k, j]:off[k, j] + lens[(0, 2, 3, 0)[k]][j]] = src[i]
        spk = np.array([int(speakers[i]) for i in keep], dtype=np.int32)
        lens_host = np.stack([lens[1], lens[2], lens[3], lens[0]])  # the rows of `off`: mel, pitch, energy, text
        with guard(device):
            up = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
            self._mel, self._pitch, self._energy, self._text, self._speaker = up(mel), up(flat[0]), up(flat[1]), up(flat[2]), up(spk)
            self._off, self._lens = up(off), up(lens_host)
        self.upload_bytes = sum(t.numel() * t.element_size() for t in (self._mel, self._pitch, self._energy, self._text, self._speaker, self._off, self._lens))
        row = lambda t, k: t.data_ptr() + k * t.shape[1] * t.element_size()  # noqa: E731
        s = NsDsStore()
        s.mel, s.pitch, s.energy, s.text, s.speaker = (t.data_ptr() for t in (self._mel, self._pitch, self._energy, self._text, self._speaker))
        s.mel_off, s.pitch_off, s.energy_off, s.text_off = (row(self._off, k) for k in range(4))
        s.mel_len, s.pitch_len, s.energy_len, s.text_len = (row(self._lens, k) for k in range(4))
        s.mel_rows, s.pitch_elems, s.energy_elems, s.text_elems = (int(off[k, N]) for k in range(4))
        s.N, s.n_mel = N, n_mel
        self._store = s
        self.launches, self.last_launches = 0, 0
        return self

    @classmethod
    def from_preprocessed(cls, filename, preprocess_config, train_config, text_to_sequence, device, max_frames=None):
        """What dataset.py:21-86 reads, once: ``filename`` (``train.txt`` / ``val.txt``: ``basename|speaker|{phonemes}|raw text`` lines) and
        ``speakers.json`` under ``preprocess_config["path"]["preprocessed_path"]``, and per utterance ``mel/``, ``pitch/`` and
        ``energy/`` ``{speaker}-{kind}-{basename}.npy``.  ``text_to_sequence(text, cleaners)`` is the caller's phoneme conversion (the
        reference's ``text.text_to_sequence``; the text front end is not part of this package).  ``train_config`` is taken as the
        reference takes it; the batch size is an argument of ``epoch()``."""
        root = preprocess_config["path"]["preprocessed_path"]
        cleaners = preprocess_config["preprocessing"].get("text", {}).get("text_cleaners", [])
        with open(os.path.join(root, "speakers.json")) as f:
            speaker_map = json.load(f)
        ids, raw, spk, texts, mels, pitches, energies = [], [], [], [], [], [], []
        with open(os.path.join(root, filename), "r", encoding="utf-8") as f:
            for line in f.readlines():
                n, s, t, r = line.strip("\n").split("|")
                if "korean_cleaners" in cleaners:  # dataset.py:37-39
                    t = t.replace(" ", "").replace("sp", ",")
                ids.append(n)
                raw.append(r)
                spk.append(speaker_map[s])
                texts.append(np.array(text_to_sequence(t, cleaners)))
                mels.append(np.load(os.path.join(root, "mel", "{}-mel-{}.npy".format(s, n))))
                pitches.append(np.load(os.path.join(root, "pitch", "{}-pitch-{}.npy".format(s, n))))
                energies.append(np.load(os.path.join(root, "energy", "{}-energy-{}.npy".format(s, n))))
        return cls.from_arrays(ids, raw, spk, texts, mels, pitches, energies, preprocess_config, device, max_frames=max_frames)

    def __len__(self):
        return len(self.ids)

    # ---- batches
    def gather(self, order_dev, order_host, first, B):
        """One batch — the utterances ``order[first : first + B]`` — as the reference's 11-tuple: ONE launch.  ``order_dev`` is the
        device int32 copy of the host int32 vector ``order_host`` (``upload_order``).  The padded axes are the batch's own maxima."""
        idx = order_host[first:first + B]
        T, P, E, L = (int(v[idx].max()) for v in (self.mel_lens, self.pitch_lens, self.energy_lens, self.text_lens))
        dev = self.device
        with guard(dev):
            new = lambda dt, *shape: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
            mels, pitches, energies = new(torch.float32, B, T, self.n_mel), new(torch.float32, B, P), new(torch.float32, B, E)
            texts, speakers, src_lens, mel_lens = new(torch.int64, B, L), new(torch.int64, B), new(torch.int64, B), new(torch.int64, B)
            o = NsDsBatch(mels.data_ptr(), pitches.data_ptr(), energies.data_ptr(), texts.data_ptr(), speakers.data_ptr(), src_lens.data_ptr(),
                          mel_lens.data_ptr(), B, T, P, E, L)
            rc = self._lib.ns_ds_gather(C.byref(self._store), C.byref(self._host_lens), _lib.ptr(order_dev), order_host.ctypes.data, order_host.size, first,
                                        C.byref(o), _lib.stream_ptr(dev))
        _lib.check(rc, "ns_ds_gather")
        self.last_launches = self._lib.ns_ds_last_launches()
        self.launches += self.last_launches
        return ([self.ids[i] for i in idx], [self.raw_texts[i] for i in idx], speakers, texts, src_lens, L, mels, mel_lens, T, pitches, energies)

    def upload_order(self, batches):
        """(device int32 order, host int32 order) of a list of index batches: the epoch's one upload (pinned, in stream order)"""
        order = np.ascontiguousarray(np.concatenate([np.asarray(b) for b in batches]).astype(np.int32))
        if order.size and (order.min() < 0 or order.max() >= len(self)):
            raise ValueError(f"an order must hold indices in [0, {len(self)})")
        with guard(self.device):
            pinned = torch.from_numpy(order).pin_memory()
            return pinned.to(self.device, non_blocking=True), order, pinned

    def epoch(self, batch_size, group_size=4, sort=True, drop_last=True, perm=None, generator=None):
        """Yields the batches of one epoch (``plan_epoch`` on the text lengths), each the reference's 11-tuple ``(ids, raw_texts, speakers,
        texts, src_lens, max_src_len, mels, mel_lens, max_mel_len, pitches, energies)``: ``max_*`` Python ints from the host lengths,
        ``ids`` / ``raw_texts`` lists, everything else a device tensor in the dtype ``to_device`` gives it.  One upload of the order
        per epoch, one launch per batch, no host read.  The reference's training loader is the default; its validation loader is
        ``validation(batch_size)``."""
        batches = plan_epoch(self.text_lens, batch_size, group_size, sort, drop_last, perm, generator)
        if not batches:
            return
        order_dev, order_host, pinned = self.upload_order(batches)  # `pinned` lives until the generator ends: it outlives the copy
        first = 0
        for b in batches:
            yield self.gather(order_dev, order_host, first, len(b))
            first += len(b)

    def validation(self, batch_size):
        """``epoch()`` as train.py's validation loader runs it: the file's order, no sorting, the tail kept (feeds ``loss.evaluate``)"""
        return self.epoch(batch_size, group_size=1, sort=False, drop_last=False, perm=np.arange(len(self)))
