"""CPU yardstick of the device-resident training set (csrc/dataset.hip through ``ns_ds_*``; smart_nar_fast_tts_amd.data): numpy only.

``collate_statement`` is the reference's ``Dataset.reprocess`` (dataset.py:88-118, with ``pad_1D`` / ``pad_2D`` of utils/tools.py) followed
by the 11-tuple branch of ``to_device`` (utils/tools.py:18-54) restated on lists of per-utterance arrays: it never sees the packed store.
``pack`` / ``gather_statement`` restate the store's layout (slots of the 1-D arrays start at multiples of four elements) and the
gather's index arithmetic on the packed arrays.  ``plan_statement`` restates train.py:30-38 + dataset.py:120-139 (groups of
``batch_size * group_size`` in the permutation's order, ``np.argsort(-len_arr)`` per group, batches, the tail) with explicit loops,
independently of ``data.plan_epoch``.

Mutants (``mutate=``), each caught on the case ``CATCHER`` names:
  padding_unwritten   the gather copies the valid elements and leaves the rest of the outputs as they were
  slot_not_rounded    a 1-D slot's offset is the plain prefix sum of the lengths (no round-up to 16 bytes)
  stable_sort         ``np.argsort(-len_arr, kind="stable")`` in place of numpy's default
  tail_kept           the partial batch at a group's end is kept although ``drop_last``"""
import numpy as np

CANARY = 0xFF  # the byte outputs are pre-filled with: a NaN as fp32, -1 as int64
MUTANTS = ("padding_unwritten", "slot_not_rounded", "stable_sort", "tail_kept")
LEVELS = ("phoneme_level", "frame_level")


# ---- synthetic utterances -------------------------------------------------------------------------------------------------------------
def _floats(rs, *shape):
    """random fp32 with some -0.0 and some denormals among them: a copy must keep their bits"""
    x = (rs.standard_normal(shape) * 2.0 - 3.0).astype(np.float32)
    kind = rs.randint(0, 16, size=shape)
    x[kind == 0] = np.float32(-0.0)
    den = (rs.randint(1, 1 << 22, size=shape).astype(np.uint32) | (rs.randint(0, 2, size=shape).astype(np.uint32) << 31)).view(np.float32)
    return np.where(kind == 1, den, x).astype(np.float32)


def make_set(lens, n_mel=80, pitch="frame_level", energy="frame_level", seed=0, n_speakers=3, vocab=300):
    """{ids, raw_texts, speakers, texts, mels, pitches, energies} of the utterances with the (L, T) of ``lens``"""
    rs = np.random.RandomState(seed)
    pick = lambda level, L, T: T if level == "frame_level" else L  # noqa: E731
    out = dict(ids=[], raw_texts=[], speakers=[], texts=[], mels=[], pitches=[], energies=[])
    for i, (L, T) in enumerate(lens):
        out["ids"].append(f"utt{i:04d}")
        out["raw_texts"].append(f"raw text {i}")
        out["speakers"].append(int(rs.randint(0, n_speakers)))
        out["texts"].append(rs.randint(1, vocab, size=L).astype(np.int64))
        out["mels"].append(_floats(rs, T, n_mel))
        out["pitches"].append(_floats(rs, pick(pitch, L, T)))
        out["energies"].append(_floats(rs, pick(energy, L, T)))
    return out


# ---- the reference's collate + to_device ----------------------------------------------------------------------------------------------
def _pad_1d(arrays, length, dtype):
    return np.stack([np.pad(np.asarray(a, dtype=dtype), (0, length - len(a)), mode="constant", constant_values=0) for a in arrays])


def collate_statement(utts, idxs, Tmax=None, Pmax=None, Emax=None, Lmax=None):
    """The 11-tuple of the reference for the utterances ``idxs`` of ``utts`` as numpy arrays in the dtypes ``to_device`` gives them
    (speakers, texts and the lengths int64; mels, pitches, energies float32).  ``Tmax`` ... widen an axis past the batch's own maximum
    (the padding is more zeros); ``max_src_len`` / ``max_mel_len`` stay the batch's own."""
    texts, mels = [utts["texts"][i] for i in idxs], [utts["mels"][i] for i in idxs]
    pitches, energies = [utts["pitches"][i] for i in idxs], [utts["energies"][i] for i in idxs]
    text_lens = np.array([t.shape[0] for t in texts], dtype=np.int64)
    mel_lens = np.array([m.shape[0] for m in mels], dtype=np.int64)
    T = max(mel_lens) if Tmax is None else Tmax
    mel = np.stack([np.pad(np.asarray(m, dtype=np.float32), ((0, T - m.shape[0]), (0, 0)), mode="constant", constant_values=0) for m in mels])
    return ([utts["ids"][i] for i in idxs], [utts["raw_texts"][i] for i in idxs], np.array([utts["speakers"][i] for i in idxs], dtype=np.int64),
            _pad_1d(texts, max(text_lens) if Lmax is None else Lmax, np.int64), text_lens, int(max(text_lens)), mel, mel_lens, int(max(mel_lens)),
            _pad_1d(pitches, max(len(p) for p in pitches) if Pmax is None else Pmax, np.float32),
            _pad_1d(energies, max(len(e) for e in energies) if Emax is None else Emax, np.float32))


TENSORS = {2: "speakers", 3: "texts", 4: "src_lens", 6: "mels", 7: "mel_lens", 9: "pitches", 10: "energies"}  # tuple position -> name


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the store and the gather on it ---------------------------------------------------------------------------------------------------
def layout(lens, rounded=True):
    """(offsets [N + 1], total) of one ragged array: slots back to back, each start rounded up to four elements when ``rounded``"""
    off, at = [], 0
    for n in lens:
        off.append(at)
        at += (int(n) + 3) // 4 * 4 if rounded else int(n)
    return np.array(off + [at], dtype=np.int64), at


def lengths(utts):
    """the four length vectors (text, mel, pitch, energy) as int32"""
    return tuple(np.array([len(a) for a in utts[k]], dtype=np.int32) for k in ("texts", "mels", "pitches", "energies"))


def pack(utts):
    """the packed store: dict(mel [sum T, n_mel] f32, pitch / energy f32 and text i32 (slots padded with a canary, never read),
    speaker i32, the four offset tables and the four length vectors)"""
    tl, ml, pl, el = lengths(utts)
    s = dict(text_len=tl, mel_len=ml, pitch_len=pl, energy_len=el, speaker=np.array(utts["speakers"], dtype=np.int32))
    s["mel_off"], rows = layout(ml, rounded=False)
    s["mel"] = np.concatenate([np.asarray(m, dtype=np.float32) for m in utts["mels"]], axis=0)
    assert s["mel"].shape[0] == rows
    for name, key, lens, dtype, fill in (("pitch", "pitches", pl, np.float32, np.float32(12345.0)), ("energy", "energies", el, np.float32, np.float32(-777.0)),
                                         ("text", "texts", tl, np.int32, np.int32(-9))):
        off, total = layout(lens)
        a = np.full(total, fill, dtype=dtype)
        for o, x in zip(off, utts[key]):
            a[o:o + len(x)] = np.asarray(x, dtype=dtype)
        s[name], s[name + "_off"] = a, off
    return s


def empty_outputs(B, Tmax, Pmax, Emax, Lmax, n_mel):
    """the seven outputs of a batch, every byte ``CANARY``"""
    f = lambda shape, dt: np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, CANARY, dtype=np.uint8).view(dt).reshape(shape)  # noqa: E731
    return dict(mels=f((B, Tmax, n_mel), np.float32), pitches=f((B, Pmax), np.float32), energies=f((B, Emax), np.float32), texts=f((B, Lmax), np.int64),
                speakers=f((B,), np.int64), src_lens=f((B,), np.int64), mel_lens=f((B,), np.int64))


def gather_statement(store, idxs, Tmax, Pmax, Emax, Lmax, mutate=None):
    """the gather on the packed store, element rule by element rule: outputs start as canaries; every element is written (the valid
    ones from the store, the rest 0) unless ``mutate`` says otherwise"""
    n_mel = store["mel"].shape[1]
    out = empty_outputs(len(idxs), Tmax, Pmax, Emax, Lmax, n_mel)
    off = {k: store[k + "_off"] for k in ("pitch", "energy", "text")}
    if mutate == "slot_not_rounded":
        off = {k: layout(store[k + "_len"], rounded=False)[0] for k in off}
    for b, i in enumerate(idxs):
        T, L = int(store["mel_len"][i]), int(store["text_len"][i])
        if mutate != "padding_unwritten":
            for k in ("mels", "pitches", "energies", "texts"):
                out[k][b] = 0
        out["mels"][b, :T] = store["mel"][store["mel_off"][i]:store["mel_off"][i] + T]
        for k, o, cap in (("pitch", "pitches", Pmax), ("energy", "energies", Emax), ("text", "texts", Lmax)):
            n = int(store[k + "_len"][i])
            out[o][b, :n] = store[k][off[k][i]:off[k][i] + n]
        out["speakers"][b], out["src_lens"][b], out["mel_lens"][b] = store["speaker"][i], L, T
    return out


def batch_maxima(store, idxs):
    """(Tmax, Pmax, Emax, Lmax) of a batch: its own maxima"""
    return tuple(int(max(store[k][i] for i in idxs)) for k in ("mel_len", "pitch_len", "energy_len", "text_len"))


# ---- the epoch's batches --------------------------------------------------------------------------------------------------------------
def plan_statement(text_lens, batch_size, group_size, sort, drop_last, perm, mutate=None):
    """the list of index batches (lists of utterance indices) one epoch of the reference's loader yields for the permutation ``perm``"""
    perm = [int(p) for p in perm]
    per_group = batch_size * group_size
    batches = []
    start = 0
    while start < len(perm):
        group = perm[start:start + per_group]  # what DataLoader hands collate_fn: the last group may be partial
        start += per_group
        if sort:
            len_arr = np.array([int(text_lens[i]) for i in group])
            pos = np.argsort(-len_arr, kind="stable") if mutate == "stable_sort" else np.argsort(-len_arr)
            group = [group[int(p)] for p in pos]
        full = len(group) // batch_size
        for k in range(full):
            batches.append(group[k * batch_size:(k + 1) * batch_size])
        rest = group[full * batch_size:]
        if rest and (not drop_last or mutate == "tail_kept"):
            batches.append(rest)
    return batches


# ---- the case table -------------------------------------------------------------------------------------------------------------------
EDGE_LENS = [(1, 1), (9, 63), (4, 64), (5, 65), (3, 17), (8, 70), (2, 1), (7, 64), (1, 65), (6, 2)]  # (L, T): the store of the kernel cases


def _case(n_mel, idxs, pitch="frame_level", energy="frame_level", wider=(0, 0, 0, 0), seed=0):
    return dict(n_mel=n_mel, idxs=list(idxs), pitch=pitch, energy=energy, wider=tuple(wider), seed=seed)


CASES = {
    "one_first": _case(80, [0]),                                      # B = 1, the first utterance of the store, T = L = 1
    "one_last": _case(80, [len(EDGE_LENS) - 1]),                      # the last utterance: its slots end the packed arrays
    "edges_80": _case(80, [1, 2, 3]),                                 # T 63, 64, 65 in one batch
    "edges_16": _case(16, [3, 0, 2], seed=1),                         # T 65, 1, 64
    "edges_4": _case(4, [1, 8, 0], seed=2),                           # one 16-byte group per row
    "repeat": _case(80, [5, 5, 4], seed=3),                           # an utterance twice in a batch
    "first_and_last": _case(16, [0, len(EDGE_LENS) - 1, 7], seed=4),
    "wider": _case(80, [4, 6, 9], wider=(7, 5, 3, 4), seed=5),        # Tmax, Pmax, Emax, Lmax above the batch's own
    "wider_one": _case(4, [6], wider=(64, 1, 1, 9), seed=6),
    "phoneme_pitch": _case(80, [1, 3, 8], pitch="phoneme_level", seed=7),        # pitch slots of 9, 5, 1 elements
    "phoneme_both": _case(16, [2, 4, 5], pitch="phoneme_level", energy="phoneme_level", seed=8),
}
CATCHER = {"padding_unwritten": "edges_80", "slot_not_rounded": "phoneme_pitch", "stable_sort": "ties_big_group", "tail_kept": "partial_last_group"}
GRID_CAPS = (1, 2)

# plan cases: (n, batch_size, group_size, lens seed); lengths in [1, 3] so that every group has ties
PLAN_CASES = {"ties_big_group": (400, 50, 4, 11), "partial_last_group": (29, 3, 4, 12), "exact_groups": (24, 3, 4, 13), "below_one_batch": (2, 3, 4, 14),
              "one_group_partial": (11, 4, 4, 15)}
PLAN_SWEEP = [(n, bs, gs) for n in (1, 2, 5, 12, 13, 29, 64) for bs in (1, 3, 4, 16) for gs in (1, 2, 4)]


def plan_case(name):
    n, bs, gs, seed = PLAN_CASES[name]
    rs = np.random.RandomState(seed)
    return dict(text_lens=rs.randint(1, 4, size=n), batch_size=bs, group_size=gs, perm=rs.permutation(n))


def case_store(name):
    """(utterances, packed store, idxs, (Tmax, Pmax, Emax, Lmax)) of a kernel case"""
    c = CASES[name]
    utts = make_set(EDGE_LENS, n_mel=c["n_mel"], pitch=c["pitch"], energy=c["energy"], seed=100 + c["seed"])
    store = pack(utts)
    caps = tuple(m + w for m, w in zip(batch_maxima(store, c["idxs"]), c["wider"]))
    return utts, store, c["idxs"], caps


def case_want(name, mutate=None):
    """the seven outputs of a case by ``gather_statement``"""
    _, store, idxs, caps = case_store(name)
    return gather_statement(store, idxs, *caps, mutate=mutate)
