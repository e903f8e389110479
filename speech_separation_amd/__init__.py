"""speech_separation_amd -- MI355X-native DPTN(-AV) separation forward path (libdptnav + thin host layer)."""
from .spec import DPRNN_AUDIO, DPRNN_AV, DPTN_AUDIO, DPTN_AV, DPTN_MASK, DPTNConfig, state_dict_spec, synthetic_inputs, synthetic_state_dict

__all__ = ["DPTNConfig", "DPTN_AV", "DPTN_AUDIO", "DPTN_MASK", "DPRNN_AUDIO", "DPRNN_AV", "DPRNNEncDec", "DPRNNAVEncDec", "state_dict_spec", "synthetic_state_dict", "synthetic_inputs",
           "DptnEngine", "DPTNAVWavEncDec", "DPTNWavEncDec", "DPTNEncDec", "ConvTasNet", "ConvTasNetEngine", "TrainableConvTasNet", "ConvTasNetTrainEngine", "DeepConvTasNet", "DeepAVConvTasNet",
           "DeepConvTasNetEngine", "TrainableDeepConvTasNet", "DeepConvTasNetTrainEngine", "TrainableDeepAVConvTasNet", "DeepAVConvTasNetTrainEngine", "FusedAdamW", "clip_grad_norm_", "SiSNRWavLoss", "MAEWavLoss",
           "MSEWavLoss", "STOIMetric", "SISDRMetric", "LipreadingEngine", "Lipreading", "ShuffleNetLipreadingEngine", "ShuffleNetLipreading", "init_lipreader", "VideoSSModel", "make_embeddings",
           "STFT", "LogMelSpectrogram", "add_spectrogram_keys", "MSESpecLoss", "L1SpecLoss",
           "VoiceFilter", "VoiceFilterEngine", "voicefilter_state_dict_spec", "voicefilter_magnitude",
           "voicefilter_analysis", "voicefilter_waveforms", "VoiceFilterSeparator", "add_magnitude_keys",
           "TrainableVoiceFilter", "VoiceFilterTrainEngine"]


def __getattr__(name):  # torch-dependent parts are imported lazily (spec.py stays numpy-only)
    if name in ("DptnEngine", "ConvTasNetEngine", "ConvTasNetTrainEngine", "DeepConvTasNetEngine",
                "DeepConvTasNetTrainEngine", "DeepAVConvTasNetTrainEngine"):
        from . import engine
        return getattr(engine, name)
    if name in ("DPTNAVWavEncDec", "DPTNWavEncDec", "DPTNEncDec", "DPRNNEncDec", "DPRNNAVEncDec", "ConvTasNet",
                "TrainableConvTasNet", "DeepConvTasNet", "DeepAVConvTasNet", "TrainableDeepConvTasNet",
                "TrainableDeepAVConvTasNet"):
        from . import model
        return getattr(model, name)
    if name in ("FusedAdamW", "clip_grad_norm_"):
        from . import optim
        return getattr(optim, name)
    if name in ("SiSNRWavLoss", "MAEWavLoss", "MSEWavLoss", "STOIMetric", "SISDRMetric", "MSESpecLoss", "L1SpecLoss"):
        from . import metrics
        return getattr(metrics, name)
    if name in ("LipreadingEngine", "Lipreading", "ShuffleNetLipreadingEngine", "ShuffleNetLipreading", "init_lipreader", "VideoSSModel", "make_embeddings"):
        from . import lipreader
        return getattr(lipreader, name)
    if name in ("STFT", "LogMelSpectrogram", "add_spectrogram_keys"):
        from . import spectral
        return getattr(spectral, name)
    if name in ("VoiceFilter", "VoiceFilterEngine", "voicefilter_state_dict_spec", "voicefilter_magnitude", "voicefilter_analysis",
                "voicefilter_waveforms", "VoiceFilterSeparator", "add_magnitude_keys", "TrainableVoiceFilter",
                "VoiceFilterTrainEngine"):
        from . import voicefilter
        return getattr(voicefilter, name)
    raise AttributeError(name)
