"""Per-phase shader-clock breakdown of the wave-balanced point-light pass (development tool).

Needs a library built with -DPBR_BAL_PROFILE=1 (make -C physically_based_renderer_amd/csrc EXTRA=...),
passed as PBR_LIB_PATH. Shades config `--config` (faithful) `--reps` times and prints the average shader
cycles per balanced wave in each phase, the pass-2 iterations per wave, and the whole kernel per wave -- once with
the product's ranking (a workgroup's 512 pixels together where all four waves run the balanced pass) and once with
per-wave ranking everywhere (PBR_RANK_PER_WAVE=1, read when the context is created); tools/rank_sim.py predicts both
iteration counts from the frame on the CPU. The unbalanced rows are stamped by shade_tile_kernel<.., 0> only: PBR_BALANCED_MIN=0 turns the balanced lists off, and
PBR_LEAN=0 keeps the pass off shade_lean_kernel, which carries no stamps (every row prints 0 without it).

    PBR_LIB_PATH=build/ab/balprof.so python tools/bal_profile.py --config 3
    PBR_LIB_PATH=build/ab/balprof.so PBR_BALANCED_MIN=0 PBR_LEAN=0 python tools/bal_profile.py --config 2
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    from clock_ramp import clock_ramp
    from physically_based_renderer_amd import _native as N
    from physically_based_renderer_amd import scenes as S
    from physically_based_renderer_amd.renderer import GBuffer, ShadingContext

    cfg = S.CONFIGS[a.config]
    planes, _ = S.fill_gbuffer_host(cfg)
    pc = S.scene_pass(cfg)
    pc.flags = int(pc.flags) | N.PBR_FLAG_FAITHFUL
    dev = torch.device("cuda", 0)
    gb = GBuffer.from_host(planes, dev)
    out = torch.empty((cfg.height, cfg.width, 4), device=dev)
    lib = N.lib()
    f = lib.pbr_debug_bal_profile
    f.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    buf = (ctypes.c_ulonglong * 16)()
    for per_wave in (False, True):
        os.environ.pop("PBR_RANK_PER_WAVE", None)
        if per_wave:
            os.environ["PBR_RANK_PER_WAVE"] = "1"
        with ShadingContext(0) as ctx:
            ctx.set_pass(pc)
            if pc.ambient_mode:
                ctx.set_env_map(S.env_map())
            clock_ramp(ctx, gb, out)
            torch.cuda.synchronize()
            assert f(buf, 1) == 0, "library not built with PBR_BAL_PROFILE"
            for _ in range(a.reps):
                ctx.shade(gb, out)
            torch.cuda.synchronize()
            assert f(buf, 1) == 0
        if report(cfg, buf, a.reps, "per-wave ranking" if per_wave else "block ranking"):
            break  # the unbalanced kernel does not rank
    os.environ.pop("PBR_RANK_PER_WAVE", None)


def report(cfg, buf, reps, ranking):
    """Prints one run's sums; True when the unbalanced kernel ran."""
    if buf[13]:  # the unbalanced kernel (PBR_BALANCED_MIN=0)
        u = buf[13]
        print(f"{cfg.name}: unbalanced faithful lean waves {u // reps} per frame")
        print(f"  entry -> light loop      {buf[11] / u:10.0f} cycles/wave")
        print(f"  light loop               {buf[12] / u:10.0f}")
        print(f"  exact re-pass barrier    {buf[14] / u:10.0f}")
        print(f"  entry -> barrier end     {buf[15] / u:10.0f}")
        return True
    waves = max(buf[4], 1)
    names = ["pass 1", "rank + exchange", "pass 2", "hand-back"]
    print(f"{cfg.name}, {ranking}: {waves // reps} balanced waves per frame")
    for i, nm in enumerate(names):
        print(f"  {nm:16s} {buf[i] / waves:10.0f} cycles/wave")
    print(f"  pass-2 iterations {buf[5] / waves:8.3f} per wave")
    print(f"  whole kernel     {buf[6] / waves:10.0f} cycles/wave (entry to the exact re-pass barrier's end)")
    print(f"  entry -> light loop      {buf[7] / waves:10.0f}")
    print(f"  loop end -> reloaded inv {buf[8] / waves:10.0f}")
    print(f"  exact re-pass barrier    {buf[9] / waves:10.0f}")
    return False


if __name__ == "__main__":
    main()
