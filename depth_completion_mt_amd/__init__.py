"""MI355X-native (gfx950) morphological depth completion: the `img_completion` cascade of
PatrizioPerugini/depth_completion_MT as hand-written HIP kernels behind a C ABI.

    from depth_completion_mt_amd import img_completion, interpolate_with_superpixels, Context
"""
from .api import (Context, DcmtError, eval_summary, evaluate_performance, img_completion, interpolate_with_superpixels,  # noqa: F401
                  make_params, reference_performance)
from . import synth  # noqa: F401

__all__ = ["Context", "DcmtError", "eval_summary", "evaluate_performance", "img_completion", "interpolate_with_superpixels",
           "make_params", "reference_performance", "synth"]
