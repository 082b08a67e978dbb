"""The reference's ``FastSpeech2Align`` on its training branch (model/fastspeech2_align.py:13-100, ``mel_lens`` given) as a
``torch.nn.Module`` whose every part is HIP in forward AND backward, and the pieces of ``train.py`` around it:

    model, optimizer = training.get_model(args, configs, device, train=True)               # utils/model.py:11-35
    Loss = FastSpeech2TrainingLoss(preprocess_config, model_config)                        # train.py:43
    losses = training.train_step(model, Loss, optimizer, batch, step, grad_acc_step, grad_clip_thresh)   # train.py:80-95
    training.save_checkpoint(model, optimizer, path)                                       # train.py:150-159
    training.fit(model, Loss, optimizer, train_set, train_config, val_set=val_set)         # train.py:59-167 over a data.DeviceDataset

The six submodules carry the reference's names in the reference's order (``stacks.TxtEncoder``, ``adaptor.VarianceAdaptor``,
``stacks.MelEncoder``, ``stacks.MelDecoder``, ``sublayers.MelLinear``, ``postnet.PostNet``), so ``state_dict()`` is a reference
checkpoint's ``"model"`` entry, key for key, and what ``save_checkpoint`` writes loads into the inference class
``model.FastSpeech2Align`` through ``checkpoint.load_checkpoint``.  With a keep-mask generator attached (``dropout.attach(model,
dropout.KeepMaskRNG(seed))``: every dropout mask of a step drawn by one HIP launch) the only torch kernels on the data path are
autograd's fan-in adds: two at ``mel`` (the mel loss, the PostNet and the residual meet there), those at ``src_output`` and those
inside the parts.  Without one, each mask is drawn with ``torch.bernoulli`` (three torch kernels per mask)."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from ._train import aligned, guard, need_gpu
from .adaptor import VarianceAdaptor
from .optim import ScheduledOptim
from .postnet import PostNet
from .stacks import Launches, MelDecoder, MelEncoder, TxtEncoder
from .sublayers import MelLinear, Prenet

KEEP_MASK_KEYS = ("txt_encoder", "mel_encoder", "prenet", "variance_adaptor", "mel_decoder", "postnet")


def _residual(p, x, book, which="forward"):
    """``ns_mh_op_residual`` on two float32 [B, T, n_mel] tensors."""
    B, T, C = p.shape
    dev = p.device
    p, x = aligned(p), aligned(x)
    with guard(dev):
        out = torch.empty_like(p)
        rc = _lib.load().ns_mh_op_residual(_lib.ptr(p), _lib.ptr(x), B * T, C, _lib.ptr(out), _lib.stream_ptr(dev))
    if book is None:
        _lib.check(rc, "ns_mh_op_residual")
    else:
        book.done(rc, which, "ns_mh_op_residual", n=1)
    return out


class _ResidualFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, x, book):
        return _residual(p.detach(), x.detach(), book)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return g, g, None  # the add passes the gradient to both operands: the same tensor, no launch


def add_residual(p, x, book=None):
    """``p + x`` (model/fastspeech2_align.py:85: ``postnet(output) + output``) in one HIP launch, out of place; the backward makes no
    launch, ``grad_output`` is the gradient of both operands.  ``p`` and ``x`` float32 [B, T, n_mel] on the GPU, equal shapes, ``n_mel``
    a multiple of 16 up to 128.  ``book`` (a ``stacks.Launches``) takes the launch count."""
    need_gpu("add_residual", "p", p)
    need_gpu("add_residual", "x", x)
    if p.dtype != torch.float32 or p.dim() != 3 or p.numel() == 0 or x.dtype != torch.float32 or tuple(x.shape) != tuple(p.shape) or x.device != p.device:
        raise ValueError(f"p and x must be non-empty float32 [B, T, n_mel] tensors of one shape on one device, got {p.dtype} {tuple(p.shape)} and "
                         f"{x.dtype} {tuple(x.shape)}")
    if torch.is_grad_enabled() and (p.requires_grad or x.requires_grad):
        return _ResidualFunction.apply(p, x, book)
    return _residual(p.detach(), x.detach(), book)


def _mask_from_lengths(lens, max_len):
    """utils/tools.py get_mask_from_lengths: bool [B, max_len], True = padded; ``max_len=None`` reads the batch maximum (one host read)."""
    if max_len is None:
        max_len = int(lens.max().item())
    return torch.arange(int(max_len), device=lens.device)[None, :] >= lens[:, None]


class FastSpeech2Align(torch.nn.Module):
    """Drop-in for ``FastSpeech2Align(preprocess_config, model_config)`` (model/fastspeech2_align.py:13-100) on the branch ``train.py``
    runs (``mel_lens`` given), forward AND backward in HIP.  ``load_state_dict(ckpt["model"], strict=True)`` takes a reference
    checkpoint; ``state_dict()`` has its keys in its order.

    ``forward(speakers, texts, src_lens, max_src_len, mels, mel_lens, max_mel_len, p_targets, e_targets, p_control=1.0,
    e_control=1.0, keep_masks=None)`` follows lines 44-100 and returns the reference's 12-tuple ``(output, postnet_output,
    p_predictions, e_predictions, log_d_predictions, d_rounded, src_masks, mel_masks, src_lens, mel_lens, tgt_alignment, d_targets)``,
    which ``FastSpeech2TrainingLoss`` takes as it is.  Both masks are built from the lengths in torch; every stack gets the lengths as
    ``lens=``, so with ``max_src_len`` and ``max_mel_len`` given the call makes no device-to-host read.  ``d_targets`` are
    ``mel_encoder.durations()`` of the last alignment map under ``no_grad`` (the reference's ``_calculate_duration`` is undefined).

    ``model_config["length_regulator"] = "gaussian"`` (the inference class's extension key) is read by the ``VarianceAdaptor``: the decoder
    is then trained on the Gaussian regulator's blended frames (``adaptor.GaussianUpsampling``, forward the inference side's launch,
    backward in HIP); the checkpoint has the same keys and loads strictly into ``model.FastSpeech2Align`` built with the same key.

    ``keep_masks`` (an extension) is a dict of dropout keep-masks handed down unchanged: ``txt_encoder`` / ``mel_encoder`` /
    ``mel_decoder`` (pairs per layer), ``prenet`` (one mask), ``variance_adaptor`` (its dict), ``postnet`` (its list).

    Raises: ``mel_lens is None`` and controls other than 1.0 (the inference path is ``model.FastSpeech2Align``), ``multi_speaker``
    (the reference class has no speaker embedding), ``decoder_hidden != 256`` (the Prenet's width), and in ``train()`` a mel longer
    than ``max_seq_len`` (the aligner would cut its maps; the reference's own forward breaks there: shorten the batch or run
    ``eval()``).

    With a ``dropout.KeepMaskRNG`` attached (``dropout.attach``), a ``train()`` forward calls its ``next_call()`` and, when
    ``max_mel_len`` is given, draws every mask of the step in one ``ns_km_draw`` (``_step_masks`` lists them in the order the forward
    consumes them); the layers then take views of that arena.  ``prefetch_keep_masks = False`` lets each layer make its own draw: the
    same bits.  Explicit ``keep_masks`` still override, part by part.

    ``launches`` / ``last_launches`` sum the parts' counters, the residual's and the generator's draws."""

    TAKES_KEEP_MASK_RNG = True   # dropout.attach() sets the generator here as well
    _keep_mask_rng = None
    prefetch_keep_masks = True   # False: every layer makes its own ns_km_draw (the same bits; the tests compare the two)

    def __init__(self, preprocess_config, model_config):
        super().__init__()
        if model_config.get("multi_speaker"):
            raise NotImplementedError("training.FastSpeech2Align: multi_speaker is not supported (the reference's FastSpeech2Align has no speaker "
                                      "embedding either); set multi_speaker to False")
        d = model_config["transformer"]["decoder_hidden"]
        if d != Prenet.D:
            raise ValueError(f"training.FastSpeech2Align: decoder_hidden must be {Prenet.D} (the aligner's Prenet is hard-coded "
                             f"{Prenet.N_MEL} -> {Prenet.D}, transformer/Layers.py:18-19), got {d}; use model.FastSpeech2Align for inference at other widths")
        self.model_config = model_config
        self.txt_encoder = TxtEncoder(model_config)
        self.variance_adaptor = VarianceAdaptor(preprocess_config, model_config)
        self.mel_encoder = MelEncoder(model_config)
        self.mel_decoder = MelDecoder(model_config)
        self.mel_linear = MelLinear(d, preprocess_config["preprocessing"]["mel"]["n_mel_channels"])
        self.postnet = PostNet()
        self.book = Launches()  # the residual add

    def _counted(self):
        return self.variance_adaptor.hip_modules() + (self.mel_linear, self.postnet)

    def _stacks(self):
        return (self.txt_encoder, self.mel_encoder, self.mel_decoder)

    @property
    def launches(self):
        """kernel launches enqueued so far by the six parts and the residual, as the C side counted them"""
        return self.book.total + sum(m.launches for m in self._counted()) + sum(s.launches for s in self._stacks())

    @property
    def last_launches(self):
        """{"forward": n, "backward": n} of the latest call (the backward once it ran)"""
        return {which: self.book.last.get(which, 0) + sum(m.last_launches.get(which, 0) for m in self._counted())
                + sum(s.last_launches[which] for s in self._stacks()) for which in ("forward", "backward")}

    def _step_masks(self, km, B, L, T_mel, T):
        """Every ``(shape, p)`` the attached generator will be asked for in this forward, in the order the forward consumes them:
        the text encoder layer by layer (attention, feed-forward), the Prenet, the aligner's layers, the predictors in the order
        the feature levels run them (k1, k2 each), the decoder's layers, the PostNet's.  ``L`` phonemes, ``T_mel`` frames of the
        reference mel and ``T`` regulated frames, each cut as its stack cuts it; a part whose masks ``km`` supplies, or that is in
        ``eval()`` or has no dropout, asks for none.  Shapes come from the arguments alone: no host read."""
        entries = []

        def site(m, p, *shapes):
            if m.training and p > 0.0:
                entries.extend((s, p) for s in shapes)

        def stack(s, rows, key):
            if km.get(key) is None:
                for layer in s.layer_stack:
                    attn = getattr(layer, s._attn)
                    site(attn, attn.p_drop, (B, rows, s.d_model))
                    site(layer.pos_ffn, layer.pos_ffn.p_drop, (B, rows, s.d_model))

        cut = lambda s, rows: min(rows, s.max_seq_len) if s.training else rows  # noqa: E731  (the train() branch of a stack slices)
        stack(self.txt_encoder, L, "txt_encoder")
        T_mel = cut(self.mel_encoder, T_mel)
        if km.get("prenet") is None:
            site(self.mel_encoder.prenet, self.mel_encoder.prenet.p_drop, (B, T_mel, Prenet.D))
        stack(self.mel_encoder, T_mel, "mel_encoder")
        va, vk = self.variance_adaptor, km.get("variance_adaptor") or {}
        rows = {"phoneme_level": L, "frame_level": T}
        order = [("duration", va.duration_predictor, L)]
        for level in ("phoneme_level", "frame_level"):
            order += [(n, p, rows[level]) for n, p, lv in (("pitch", va.pitch_predictor, va.pitch_feature_level),
                                                         ("energy", va.energy_predictor, va.energy_feature_level)) if lv == level]
        for name, pred, r in order:
            if vk.get(name) is None:
                site(pred, pred.dropout, *[(B, r, pred.filter_size)] * 2)
        T = cut(self.mel_decoder, T)
        stack(self.mel_decoder, T, "mel_decoder")
        if km.get("postnet") is None:
            site(self.postnet, self.postnet.dropout, *[(B, T, c) for c in self.postnet.channels[1:]])
        return entries

    def forward(self, speakers, texts, src_lens, max_src_len, mels=None, mel_lens=None, max_mel_len=None, p_targets=None, e_targets=None,
                p_control=1.0, e_control=1.0, keep_masks=None):
        if mel_lens is None or mels is None:
            raise NotImplementedError("training.FastSpeech2Align is the training branch (fastspeech2_align.py:55-58): mels and mel_lens must be "
                                      "given.  Synthesis without a reference mel is model.FastSpeech2Align (the inference path).")
        if (p_control, e_control) != (1.0, 1.0):
            raise NotImplementedError("the controls scale predictions on the inference path only (model.FastSpeech2Align); with targets given they must be 1.0")
        if self.training and mels.shape[1] > self.mel_encoder.max_seq_len:
            raise ValueError(f"training.FastSpeech2Align: in train() the mel must not exceed max_seq_len = {self.mel_encoder.max_seq_len} frames, got "
                             f"{mels.shape[1]} (the aligner would cut its maps and the durations with them); shorten the batch, or run eval()")
        km = keep_masks or {}
        unknown = set(km) - set(KEEP_MASK_KEYS)
        if unknown:
            raise ValueError(f"keep_masks takes the keys {KEEP_MASK_KEYS}, got {sorted(unknown)}")
        need_gpu("FastSpeech2Align", "texts", texts)
        self.book.begin()
        for m in self._counted():
            m.last_launches = {}
        rng = self._keep_mask_rng if self.training else None
        if rng is not None:  # one draw counter per step; all its masks in one launch where the shapes are known without a host read
            drawn = rng.launches
            rng.next_call()
            if self.prefetch_keep_masks and max_mel_len is not None:
                rng.prefetch(self._step_masks(km, texts.shape[0], texts.shape[1], mels.shape[1], int(max_mel_len)), texts.device)

        src_masks = _mask_from_lengths(src_lens, max_src_len)
        mel_masks = _mask_from_lengths(mel_lens, max_mel_len)

        src_output = self.txt_encoder(texts, src_masks, lens=src_lens, keep_masks=km.get("txt_encoder"))

        tgt_output, tgt_alignment = self.mel_encoder(src_output, mels, src_masks, mel_masks, src_lens=src_lens, mel_lens=mel_lens,
                                                     keep_masks=km.get("mel_encoder"), prenet_keep_mask=km.get("prenet"))
        with torch.no_grad():
            d_targets = self.mel_encoder.durations(tgt_alignment[-1], src_lens, mel_lens)

        (output, p_predictions, e_predictions, log_d_predictions, d_rounded, mel_lens_out, mel_masks) = self.variance_adaptor(
            src_output, src_masks, mel_masks, max_mel_len, p_targets, e_targets, d_targets, p_control, e_control,
            keep_masks=km.get("variance_adaptor"))

        output, mel_masks = self.mel_decoder(output, mel_masks, lens=mel_lens, keep_masks=km.get("mel_decoder"))
        output = self.mel_linear(output)

        postnet_output = add_residual(self.postnet(output, keep_masks=km.get("postnet")), output, book=self.book)
        if rng is not None:
            self.book.done(0, "forward", "ns_km_draw", n=rng.launches - drawn)

        return (output, postnet_output, p_predictions, e_predictions, log_d_predictions, d_rounded, src_masks, mel_masks, src_lens, mel_lens_out,
                tgt_alignment, d_targets)


    def forward_teacher_forced(self, *args, async_status=False, **kwargs):
        """What ``loss.evaluate`` calls on a model: this module's own forward under ``no_grad`` as a ``model.ForwardOutput`` with no
        status words (a token id outside the vocabulary raises in the embedding here, and nothing is ever cut off), so ``check()``
        has nothing to read.  Run it in ``eval()``; ``async_status`` is accepted and changes nothing."""
        from .model import ForwardOutput

        with torch.no_grad():
            return ForwardOutput(self(*args, **kwargs))


def get_model(args, configs, device, train=True):
    """utils/model.py:11-35 for the training case: ``(model, ScheduledOptim)``, both restored from
    ``{ckpt_path}/{restore_step}.pth.tar`` when ``args.restore_step`` is nonzero, the model in ``train()``."""
    if not train:
        raise NotImplementedError("training.get_model builds the trainable model; for inference use checkpoint.get_model(args, configs, device)")
    preprocess_config, model_config, train_config = configs
    model = FastSpeech2Align(preprocess_config, model_config).to(device)
    ckpt = None
    if args.restore_step:
        path = os.path.join(train_config["path"]["ckpt_path"], "{}.pth.tar".format(args.restore_step))
        # weights_only: a checkpoint is tensors + an optimizer state dict; do not unpickle arbitrary objects
        ckpt = torch.load(path, map_location=device, weights_only=True)
        model.load_state_dict(ckpt["model"], strict=True)
    scheduled_optim = ScheduledOptim(model, train_config, model_config, args.restore_step)
    if ckpt is not None:
        scheduled_optim.load_state_dict(ckpt["optimizer"])
    model.train()
    return model, scheduled_optim


def train_step(model, loss, optimizer, batch, step, grad_acc_step, grad_clip_thresh, keep_masks=None):
    """train.py:80-95 for one batch (the reference's tuple: ids, raw texts, then the nine arguments of ``forward``): forward, loss,
    ``(total / grad_acc_step).backward()`` and, when ``step % grad_acc_step == 0``, the clip, the Adam step, the schedule and the
    zeroing of the gradients in ``optimizer.step_and_update_lr(grad_clip_thresh, zero_grad=True)``.  Returns the seven loss tensors
    (device, 0-dim) and reads nothing to the host.  ``keep_masks`` (an extension) goes to the model."""
    output = model(*(batch[2:]), keep_masks=keep_masks)
    losses = loss(batch, output)
    (losses[0] / grad_acc_step).backward()
    if step % grad_acc_step == 0:
        optimizer.step_and_update_lr(grad_clip_thresh, zero_grad=True)
    return losses


def save_checkpoint(model, optimizer, path, rng=None):
    """train.py:150-159: ``{"model": model.state_dict(), "optimizer": optimizer._optimizer.state_dict()}`` written to ``path``.  The
    schedule's learning rate is a numpy float64 (model/optimizer.py:20 computes it with ``np.power``); it is written as the Python float
    of the same value, so that ``torch.load(..., weights_only=True)`` — what ``checkpoint.load_checkpoint`` and ``get_model`` use —
    takes the file.

    ``rng`` (an extension; a ``dropout.KeepMaskRNG``) adds a third key, ``"keep_mask_rng"``: its ``state_dict()``, plain ints.  A run
    resumed with ``rng.load_state_dict(torch.load(path, weights_only=True)["keep_mask_rng"])`` draws the masks the saved run would
    have drawn next.  Without ``rng`` the file has the two keys it always had."""
    def plain(v):
        if isinstance(v, (list, tuple)):
            return type(v)(plain(x) for x in v)
        return v.item() if isinstance(v, np.generic) else v

    opt = optimizer._optimizer.state_dict()
    opt["param_groups"] = [{k: plain(v) for k, v in g.items()} for g in opt["param_groups"]]
    ckpt = {"model": model.state_dict(), "optimizer": opt}
    if rng is not None:
        ckpt["keep_mask_rng"] = rng.state_dict()
    torch.save(ckpt, path)


def fit(model, loss, optimizer, train_set, train_config, restore_step=0, val_set=None, rng=None, on_log=None):
    """train.py:59-167 without tensorboard, tqdm and synthesis, over a ``data.DeviceDataset``: epochs of
    ``train_set.epoch(batch_size)`` (a new ``torch.randperm`` each), one ``train_step`` per batch, steps counted from
    ``restore_step + 1``; returns the last step, ``train_config["step"]["total_step"]``, once it has run.

    Every ``log_step`` steps the seven losses are read (the loop's only host read) and handed to ``on_log(step, losses, "train")`` as
    floats.  Every ``val_step`` steps, with a ``val_set``: ``model.eval()``, ``loss.evaluate(model, val_set.validation(batch_size),
    loss)``, ``model.train()``, and the seven means go to ``on_log(step, means, "val")``.  Every ``save_step`` steps:
    ``save_checkpoint(model, optimizer, "{ckpt_path}/{step}.pth.tar", rng=rng)``.  ``rng`` (a ``dropout.KeepMaskRNG``) is only saved
    here: attach it to the model with ``dropout.attach``.  A loop over existing calls: it adds no arithmetic."""
    from .loss import evaluate

    opt, every = train_config["optimizer"], train_config["step"]
    batch_size, grad_acc_step, grad_clip_thresh = opt["batch_size"], opt["grad_acc_step"], opt["grad_clip_thresh"]
    total_step = every["total_step"]
    step = int(restore_step) + 1
    if step > total_step:
        raise ValueError(f"fit: restore_step {restore_step} is not below total_step {total_step}")
    if batch_size > len(train_set):
        raise ValueError(f"fit: batch_size {batch_size} exceeds the {len(train_set)} utterances of the set: no epoch would hold a batch")
    while True:
        for batch in train_set.epoch(batch_size):
            losses = train_step(model, loss, optimizer, batch, step, grad_acc_step, grad_clip_thresh)
            if step % every["log_step"] == 0:
                values = torch.stack([v.detach() for v in losses]).cpu().tolist()
                if on_log is not None:
                    on_log(step, values, "train")
            if val_set is not None and step % every["val_step"] == 0:
                model.eval()
                means = evaluate(model, val_set.validation(batch_size), loss)
                model.train()
                if on_log is not None:
                    on_log(step, list(means), "val")
            if step % every["save_step"] == 0:
                os.makedirs(train_config["path"]["ckpt_path"], exist_ok=True)
                save_checkpoint(model, optimizer, os.path.join(train_config["path"]["ckpt_path"], "{}.pth.tar".format(step)), rng=rng)
            if step == total_step:
                return step
            step += 1
