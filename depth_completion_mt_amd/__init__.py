"""MI355X-native (gfx950) morphological depth completion: the `img_completion` cascade of
PatrizioPerugini/depth_completion_MT as hand-written HIP kernels behind a C ABI.

    from depth_completion_mt_amd import img_completion, interpolate_with_superpixels, Context
"""
from .api import (Context, DcmtError, eval_summary, evaluate_performance, img_completion, interpolate_with_superpixels,  # noqa: F401
                  make_params, reference_performance, to_color_image)
from . import synth  # noqa: F401

__all__ = ["Context", "DcmtError", "eval_summary", "evaluate_performance", "img_completion", "interpolate_with_superpixels",
           "make_params", "reference_performance", "synth", "to_color_image", "JET_BGR"]


def __getattr__(name):
    if name == "JET_BGR":                        # loads the library on first use (api.JET_BGR)
        from . import api
        return api.JET_BGR
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
