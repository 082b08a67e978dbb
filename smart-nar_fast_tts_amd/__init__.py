"""MI355X-native FastSpeech2 inference forward (drop-in for the reference's
``FastSpeech2Align.forward`` path, model/fastspeech2_align.py:30-100).

Submodules are imported lazily: ``workload`` is pure numpy and importable
anywhere; ``model`` / ``ops`` need the HIP C-ABI library and fail loudly
when it is missing.  ``FastSpeech2Loss``, ``FastSpeech2TrainingLoss`` and ``evaluate`` (``loss``), ``TacotronSTFT``, ``get_mel_from_wav``,
``STFT``, ``griffin_lim``, ``mel_to_wave`` and ``inv_mel_spec`` (``audio``), ``VarianceTargets`` (``targets``), ``ScheduledOptim`` (``optim``), the trainable ``VariancePredictor`` (``predictor``), ``MultiHeadAttention`` / ``MultiHeadCrossAttention`` / ``PositionwiseFeedForward`` / ``FFTBlock`` / ``Prenet`` / ``FFTBlock2`` (``sublayers``) the trainable ``PostNet`` (``postnet``) and the trainable ``VarianceAdaptor`` with its ``VarianceEmbedding``, ``LengthRegulator`` and ``GaussianUpsampling`` (``adaptor``) and the trainable ``TxtEncoder`` / ``MelDecoder`` / ``MelEncoder`` stacks with their ``WordEmbedding`` and ``mask_rows`` (``stacks``), the trainable ``MelLinear`` (``sublayers``) and the ``training`` module (the trainable ``FastSpeech2Align``, ``get_model``, ``train_step``, ``save_checkpoint``, ``add_residual``) and the ``dropout`` module (``KeepMaskRNG``, ``attach``, ``detach``: dropout keep-masks from a counter-based generator in HIP) and the ``data`` module (``DeviceDataset``, ``plan_epoch``: the training set resident on the device, a batch per gather launch) resolve on first use."""
__all__ = ["workload", "FastSpeech2Loss", "FastSpeech2TrainingLoss", "evaluate", "TacotronSTFT", "get_mel_from_wav", "STFT", "griffin_lim", "mel_to_wave", "inv_mel_spec", "VarianceTargets", "ScheduledOptim", "VariancePredictor", "MultiHeadAttention", "MultiHeadCrossAttention", "PositionwiseFeedForward", "FFTBlock", "Prenet", "FFTBlock2", "PostNet", "VarianceAdaptor", "VarianceEmbedding", "LengthRegulator", "GaussianUpsampling", "TxtEncoder", "MelDecoder", "MelEncoder", "WordEmbedding", "mask_rows", "MelLinear", "training", "dropout", "KeepMaskRNG", "data", "DeviceDataset"]


def __getattr__(name):
    if name in ("FastSpeech2Loss", "FastSpeech2TrainingLoss", "evaluate"):
        from . import loss

        return getattr(loss, name)
    if name in ("TacotronSTFT", "get_mel_from_wav", "STFT", "griffin_lim", "mel_to_wave", "inv_mel_spec"):
        from . import audio

        return getattr(audio, name)
    if name == "VarianceTargets":
        from . import targets

        return targets.VarianceTargets
    if name == "ScheduledOptim":
        from . import optim

        return optim.ScheduledOptim
    if name == "VariancePredictor":
        from . import predictor

        return predictor.VariancePredictor
    if name == "training":  # the trainable FastSpeech2Align, get_model, train_step, save_checkpoint, add_residual
        import importlib

        return importlib.import_module(".training", __name__)
    if name == "dropout":  # KeepMaskRNG, attach, detach
        import importlib

        return importlib.import_module(".dropout", __name__)
    if name == "data":  # DeviceDataset, plan_epoch
        import importlib

        return importlib.import_module(".data", __name__)
    if name == "DeviceDataset":
        from . import data

        return data.DeviceDataset
    if name == "KeepMaskRNG":
        from . import dropout

        return dropout.KeepMaskRNG
    if name in ("MultiHeadAttention", "MultiHeadCrossAttention", "PositionwiseFeedForward", "FFTBlock", "Prenet", "FFTBlock2", "MelLinear",
                "set_ffn_matmul"):
        from . import sublayers

        return getattr(sublayers, name)
    if name == "PostNet":
        from . import postnet

        return postnet.PostNet
    if name in ("VarianceAdaptor", "VarianceEmbedding", "LengthRegulator", "GaussianUpsampling"):
        from . import adaptor

        return getattr(adaptor, name)
    if name in ("TxtEncoder", "MelDecoder", "MelEncoder", "WordEmbedding", "mask_rows"):
        from . import stacks

        return getattr(stacks, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
