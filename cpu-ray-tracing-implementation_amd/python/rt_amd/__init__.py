"""Python handle on the MI355X wavefront path tracer (C ABI: include/rt_hip.h)."""
from . import abi
from .render import Context, Multi, adaptive_variance, denoise_host, multi_plan, plan_kernel, plan_radiance_kernel
from .scene import SceneBuilder, perspective

__all__ = ["abi", "Context", "Multi", "adaptive_variance", "denoise_host", "multi_plan", "plan_kernel", "plan_radiance_kernel", "SceneBuilder", "perspective"]
