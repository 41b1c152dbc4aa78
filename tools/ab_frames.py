"""Same-frames A/B of kernel builds on the rare- and special-normal case table (development tool).

    python tools/ab_frames.py --libs A.so B.so [...]

Shades the frames of tests/ibl_path_cases.py (every rare or special normal of the diffuse-IBL ambient in the first
element of a pixel pair, the second, and both; 24, 8 and 0 point lights; the Chelsea map and the 1x1, 2x1, 3x2 maps;
exact and faithful mode) with each library of --libs, each in a fresh child process (one libpbrshade.so per process,
PBR_LIB_PATH), and prints per frame a checksum of the fp32 bit patterns and the pass statistics. The summary says
whether every library produced the first one's checksums and statistics. tools/ab_bench.py compares the scene
configs, whose normals hit none of the patched cases; this shows the patched paths unchanged.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(lib: str) -> None:
    os.environ["PBR_LIB_PATH"] = os.path.abspath(lib)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch

    import ibl_path_cases as C
    from physically_based_renderer_amd.renderer import ShadingContext

    dev = torch.device("cuda", 0)
    envs = C.env_maps()
    with ShadingContext(0) as ctx:
        for label, p, _ in C.frames():
            for n_point in C.LIGHT_COUNTS:
                for name, env in envs.items():
                    for mode in ("exact", "faithful"):
                        got, st, kernel = C.shade_case(ctx, dev, p, n_point, mode == "faithful", env)
                        bits = got.view(np.uint32).astype(np.uint64).ravel()
                        csum = int((bits * (np.arange(bits.size, dtype=np.uint64) % 65521 + 1)).sum() % (1 << 61))
                        print(json.dumps({"frame": label, "lights": n_point, "env": name, "mode": mode,
                                          "checksum": csum, "nan": int(np.isnan(got).sum()),
                                          "exact_pixels": st["exact_pixels"], "light_terms": st["light_terms"],
                                          "geometry_pixels": st["geometry_pixels"], "kernel": kernel}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+", required=True)
    ap.add_argument("--one", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one)
        return
    results = {}
    for lib in a.libs:
        p = subprocess.run([sys.executable, __file__, "--libs", lib, "--one", lib], capture_output=True, text=True,
                           timeout=600)
        if p.returncode != 0:
            print(p.stdout, p.stderr, file=sys.stderr)
            raise SystemExit(f"{lib}: exit {p.returncode}")
        rows = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        results[lib] = rows
        for r in rows:
            print(json.dumps({"lib": lib, **r}), flush=True)
    first = results[a.libs[0]]
    print(f"summary: {len(first)} frames per library")
    fail = False
    for lib in a.libs[1:]:
        diff = [(x, y) for x, y in zip(first, results[lib]) if x != y]
        fail |= bool(diff) or len(results[lib]) != len(first)
        print(f"  {lib}: {len(first) - len(diff)} of {len(first)} frames == {a.libs[0]} "
              f"(checksum, NaN count, pass statistics, kernel)")
        for x, y in diff[:10]:
            print(f"    differs: {x} vs {y}")
    raise SystemExit(1 if fail else 0)


if __name__ == "__main__":
    main()
