"""The path kernels by name: the traversal part of the tag Context.last_kernel() reports and rt_amd.plan_kernel plans,
with the precision left open ("{p}": f32 or f64), and all_tags(), every tag a render can launch. Shared by the two GPU
tables (test_gpu_lights.py, test_gpu_materials.py) and the CPU tests of the choice (test_plan.py, test_plan_tables.py)."""

FLAT_LL, FLAT_LDS, FLAT_GLOBAL = "FlatTrav<{p},1,1>", "FlatTrav<{p},1,0>", "FlatTrav<{p},0,0>"
LIN_QUAD, LIN_LLI, LIN_VOL = "LinearTrav<{p},0,0,0,0>", "LinearTrav<{p},0,0,1,1>", "LinearTrav<{p},0,0,1,0>"
LIN_SPH, LIN_ALL = "LinearTrav<{p},1,0,0,0>", "LinearTrav<{p},1,1,1,0>"
# WideTrav<R, SPH, TRI, QUAD, MOV, tree in LDS, LL, NL>
W_SPH_NL, W_SPH_NL_HBM = "WideTrav<{p},1,0,0,0,1,0,1>", "WideTrav<{p},1,0,0,0,0,0,1>"
W_SPH, W_SPH_HBM = "WideTrav<{p},1,0,0,0,1,0,0>", "WideTrav<{p},1,0,0,0,0,0,0>"
W_TRI, W_TRI_HBM = "WideTrav<{p},0,1,0,0,1,0,0>", "WideTrav<{p},0,1,0,0,0,0,0>"
W_TQ, W_TQ_HBM = "WideTrav<{p},0,1,1,0,1,0,0>", "WideTrav<{p},0,1,1,0,0,0,0>"
W_TQ_LL, W_TQ_LL_HBM = "WideTrav<{p},0,1,1,0,1,1,0>", "WideTrav<{p},0,1,1,0,0,1,0>"
W_ALL, W_ALL_HBM = "WideTrav<{p},1,1,1,1,1,0,0>", "WideTrav<{p},1,1,1,1,0,0,0>"


def all_tags():
    """Every tag launch_step can launch (rt_kernels.hip launch_step's list of instantiations), 96 in all."""
    tags = set()
    for p in ("f32", "f64"):
        # the flat program has no extended form; its LDS forms exist in the persistent schedule only
        tags |= {f"FlatTrav<{p},1,1> persist", f"FlatTrav<{p},1,0> persist", f"FlatTrav<{p},0,0> persist",
                 f"FlatTrav<{p},0,0> step"}
        for trav in (LIN_QUAD, LIN_VOL, LIN_SPH, LIN_ALL):
            tags |= {trav.format(p=p) + camx + sched for camx in ("", " camx") for sched in (" persist", " step")}
        tags |= {LIN_LLI.format(p=p) + camx + " persist" for camx in ("", " camx")}  # LLI: persist_body's shade only
        # the wide tree: the persistent schedule and the perspective camera only (rt_plan.h kernel_family)
        tags |= {w.format(p=p) + " persist" for w in (W_SPH_NL, W_SPH_NL_HBM, W_SPH, W_SPH_HBM, W_TRI, W_TRI_HBM, W_TQ,
                                                       W_TQ_HBM, W_TQ_LL, W_TQ_LL_HBM, W_ALL, W_ALL_HBM)}
        stacks = ["8,0", "16,0", "32,0"] + (["16,1"] if p == "f32" else [])
        tags |= {f"StackTrav<{p},{s}>" + camx + sched for s in stacks for camx in ("", " camx")
                 for sched in (" persist", " step")}
    return tags
