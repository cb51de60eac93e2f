"""Which kernel does each ``tile=(bm, bn, variant)`` launch?  Numerics cannot tell two forms of
one kernel apart (variant 9 computes what variant 8 computes); the dispatched kernel's name can.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python scripts/conv_dispatch_names.py
    python scripts/conv_dispatch_names.py --names DIR > names.txt          # conv kernels, launch order
    python scripts/conv_dispatch_names.py --compare a.txt b.txt            # exit 1 if they differ

The run launches every (bm, bn, variant) of ``ops.conv.VARIANTS`` once, in table order, through
``conv2d(..., tile=)`` only, so the same file runs on a tree from before the table existed: it
carries its own copy of the list and checks it against the table when there is one.
"""
import argparse
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T4 = ((128, 128), (128, 64), (64, 128), (64, 64))
# variant -> [(shape name, tiles)]
PLAN = {
    0: [("main", T4), ("narrow", ((128, 32), (256, 32)))],
    1: [("main", T4), ("n80", ((128, 80), (256, 80)))],
    2: [("main", T4 + ((256, 128), (128, 256), (256, 64)))],
    3: [("main", ((64, 64), (64, 128), (128, 64)))],
    4: [("main", ((64, 128),))],
    5: [("main", ((128, 128), (128, 64), (64, 128), (256, 128), (128, 256)))],
    6: [("main", ((256, 128), (128, 256)))],
    7: [("narrow", ((8, 32), (16, 32), (8, 64), (16, 64)))],
    8: [("main", ((256, 256), (256, 128), (128, 256), (256, 64), (128, 128)))],
    9: [("main", ((128, 128), (256, 64), (128, 64), (64, 128), (64, 64)))],
    10: [("patch", ((8, 64),))],
    11: [("main", ((256, 256), (256, 128), (128, 256)))],
    12: [("pw", ((128, 128),))],
    13: [("pw", ((64, 128),)), ("dual", ((64, 128),))],
    14: [("pw", ((64, 128),))],
    16: [("patchw", ((392, 128),))],
    17: [("rows", ((1, 32),))],
    18: [("n80_64", ((256, 80), (128, 80))), ("n144", ((256, 144), (128, 144)))],
    19: [("main", ((128, 128), (128, 256)))],
    # with a residual the persistent walk has no 256 x 256 form (the tuner never offers it)
    20: [("main", ((256, 128), (128, 256))), ("main_nores", ((256, 256), (256, 128), (128, 256)))],
}


def run():
    import torch
    from aiko_services_amd import ops
    from aiko_services_amd.ops import conv as C
    ops.require_native()
    if hasattr(C, "VARIANTS"):
        for v, info in C.VARIANTS.items():
            mine = [t for _, tiles in PLAN[int(v)] for t in tiles]
            assert sorted(set(mine)) == sorted(set(info.tiles)), (v, mine, info.tiles)
        assert len(PLAN) == len(C.VARIANTS)
    dev = "cuda"
    g = torch.Generator().manual_seed(0)

    def x(*shape):
        return torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)

    def spec(cin, cout, k, **kw):
        w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
        return C.make_conv_spec(w, torch.zeros(cout), pad=k // 2, act="relu", device=dev, **kw)

    main = spec(128, 256, 3)
    rows_buf = x(2, 8, 80, 64)
    shapes = {   # name -> kwargs of conv2d
        "main": dict(x=x(2, 28, 28, 128), spec=main, residual=x(2, 28, 28, 256)),
        "main_nores": dict(x=x(2, 28, 28, 128), spec=main),
        "narrow": dict(x=x(2, 20, 20, 32), spec=spec(32, 32, 3)),
        "n80": dict(x=x(2, 20, 20, 80), spec=spec(80, 80, 3)),
        "n80_64": dict(x=x(2, 20, 20, 64), spec=spec(64, 80, 3)),
        "n144": dict(x=x(2, 20, 20, 64), spec=spec(64, 144, 3)),
        "patch": dict(x=x(2, 56, 56, 64), spec=spec(64, 64, 3)),
        "patchw": dict(x=x(2, 28, 28, 128), spec=spec(128, 128, 3)),
        "rows": dict(x=rows_buf[..., :32], spec=spec(32, 32, 3), residual=rows_buf[..., 32:]),
        "pw": dict(x=x(3, 14, 14, 256), spec=spec(256, 1024, 1), residual=x(3, 14, 14, 1024)),
        "dual": dict(x=x(2, 28, 28, 128), x2=x(2, 56, 56, 256),
                     spec=C.fuse_shortcut(spec(128, 512, 1), spec(256, 512, 1, stride=2))),
    }
    torch.cuda.synchronize()
    n = 0
    for v, parts in PLAN.items():
        for shape, tiles in parts:
            for bm, bn in tiles:
                C.conv2d(tile=(bm, bn, v), **shapes[shape])
                torch.cuda.synchronize()
                print(f"{shape} ({bm}, {bn}, {v})", flush=True)
                n += 1
    print(f"launched {n} (bm, bn, variant) forms")


def names(trace_dir):
    """Conv kernel names of a ``--kernel-trace --output-format csv`` run, in dispatch order."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    with open(files[0], newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    return [r["Kernel_Name"] for r in rows if "conv" in r["Kernel_Name"] and "aiko" in r["Kernel_Name"]]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--names", metavar="DIR", help="print the conv kernel names of a trace directory")
    ap.add_argument("--compare", nargs=2, metavar="FILE", help="compare two --names listings")
    a = ap.parse_args()
    if a.names:
        print("\n".join(names(a.names)))
    elif a.compare:
        la, lb = (open(p).read().splitlines() for p in a.compare)
        diff = [(i, p, q) for i, (p, q) in enumerate(zip(la, lb)) if p != q]
        print(f"{len(la)} vs {len(lb)} dispatches, {len(diff)} differ")
        for i, p, q in diff[:20]:
            print(f"  #{i}: {p}\n   vs {q}")
        sys.exit(0 if la == lb else 1)
    else:
        run()


if __name__ == "__main__":
    main()
