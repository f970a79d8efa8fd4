"""Python handle on the MI355X wavefront path tracer (C ABI: include/rt_hip.h)."""
from . import abi
from .render import (Context, Multi, TemporalAccumulator, adaptive_variance, denoise_host, history_planes, multi_plan,
                     plan_kernel, plan_radiance_kernel, temporal_host)
from .scene import SceneBuilder, perspective

__all__ = ["abi", "Context", "Multi", "adaptive_variance", "denoise_host", "history_planes", "multi_plan", "temporal_host", "TemporalAccumulator", "plan_kernel", "plan_radiance_kernel", "SceneBuilder", "perspective"]
