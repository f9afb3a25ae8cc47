"""Host-side mirror of the reference's ``core/gdrn_modeling`` inference surface:
``build_model_optimizer(cfg, is_test)``, ``GDRN_DoubleMask.forward`` and the evaluator-style
post-processing, with the per-ROI CPU / GL work replaced by calls into ``libgdrnpp_hip.so``."""

__all__ = ["YoloGdrnPredictor"]


def __getattr__(name):
    # resolved on first use: predictor.py imports the detector package, which itself imports hip_layers from this one
    if name == "YoloGdrnPredictor":
        from .predictor import YoloGdrnPredictor

        return YoloGdrnPredictor
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
