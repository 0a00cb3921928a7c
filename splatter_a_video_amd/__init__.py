"""splatter_a_video_amd -- MI355X (gfx950) native differentiable video-Gaussian rasterizer.

Drop-in for the reference's ``dptr.gs`` operator package: hand-written HIP kernels in
``csrc/`` behind the C ABI of ``include/splat_hip.h``, reached through ctypes.  See DESIGN.md.
"""
from . import gs  # noqa: F401
from .edit import AppearanceFit, fit_appearance, select_gaussians  # noqa: F401
from .layers import Layer, LayeredClip, add_foreground, foreground_mask, render_part  # noqa: F401
from .lift import FeatureLift, blend_lift, lift_features  # noqa: F401
from .flow import flow_attribute, flow_epe, flow_occlusion, flow_to_image, render_flow, warp_by_flow  # noqa: F401

__version__ = "0.1.0"
