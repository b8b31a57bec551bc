"""Training iterations at the VG shape in fp32 and bf16 mode, against another build of the library -- for profiles/train_bf16_bench.md.

  python tools/train_bf16_bench.py --parent DIR      the comparison: DIR holds a built checkout of the parent commit.  Three rounds of
        [parent fp32, this tree fp32, this tree bf16], the order rotated from round to round, every run a fresh child process under
        its own time limit; then
        this tree's weight-gradient kernels at the four VG level shapes.  One JSON line per run, a summary at the end.
  python tools/train_bf16_bench.py --child fp32|bf16 one run of the tree this file is in (the parent has no precision argument: fp32
        there runs without it): B = 64, `giou` loss, TB_ITERS iterations after 3 warm-up ones, with and without the self-conditioning
        pass (coin forced).  Host clock around an iteration that ends in a device synchronise.
  python tools/train_bf16_bench.py --child kernels   dW = dy^T x at the shapes of fc1 on the four VG levels through dsg_debug_t_gemm
        (fp32: gemm_tn_f32_kernel) and dsg_debug_t_gemm_lp (gemm_tn_bf16_kernel), device events around TB_KREP hook calls -- kernel
        plus split-K reduction plus the hook's synchronise, so small shapes are overstated.
TB_ITERS=10 TB_KREP=10 TB_BATCH=64"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def child_iterations(precision):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from diffusesg_amd import synth as Y, weights as W
    from diffusesg_amd.model import build_network
    from diffusesg_amd.train import AdamHip, EMAHip, NodeAdjEDMObjectiveGeneratorHip, NodeAdjRainbowLossHip, train_one_iteration
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    B, n_it = int(os.environ.get("TB_BATCH", "64")), int(os.environ.get("TB_ITERS", "10"))
    cfg, flags, ca, cn, rnd, ea, en, coin = Y.train_case("vg", B=B)
    model = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    gen = NodeAdjEDMObjectiveGeneratorHip(precond="edm", sigma_dist="edm", other_params=None, dev="cuda", symmetric_noise=False)
    lf = NodeAdjRainbowLossHip(edge_loss_weight=1.0, node_loss_weight=1.0, flag_reweight=False, objective="edm")
    opt, emas = AdamHip(model), [EMAHip(model, beta=0.9999)]
    a, x, f = T(ca), T(cn), T(flags)
    kw = {} if precision is None else {"precision": precision}
    out = {"precision": precision or "fp32", "B": B, "iters": n_it}
    real = np.random.rand
    try:
        for label, forced in (("no_sc", 0.9), ("sc", 0.1)):
            np.random.rand = lambda *a_: forced
            ts = []
            for it in range(n_it + 3):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                loss, *_ = train_one_iteration(model, gen, lf, opt, emas, a, x, f, iou_loss_weight=1.0, iou_loss_type="giou", **kw)
                torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
            ts = ts[3:]
            out[label + "_mean_s"], out[label + "_min_s"], out[label + "_loss"] = float(np.mean(ts)), float(min(ts)), float(loss)
    finally:
        np.random.rand = real
    print("TBJSON " + json.dumps(out), flush=True)


def child_kernels():
    sys.path.insert(0, ROOT)
    import torch
    from diffusesg_amd import lib as L
    lib = L.load()
    rep = int(os.environ.get("TB_KREP", "10"))
    B = int(os.environ.get("TB_BATCH", "64"))
    p = lambda t: C.c_void_p(t.data_ptr())
    for level, (rows, Cc) in enumerate(((B * 4096, 96), (B * 1024, 192), (B * 256, 384), (B * 64, 768))):
        out_, in_ = 4 * Cc, Cc                                    # fc1: dW [4C, C] = d_pre^T xn2
        dy, xx = torch.randn(rows, out_, device="cuda"), torch.randn(rows, in_, device="cuda")
        dW, db = torch.empty(out_, in_, device="cuda"), torch.empty(out_, device="cuda")
        res = {"level": level, "tokens": rows, "out": out_, "in": in_, "flop": 2.0 * rows * out_ * in_}
        for name in ("fp32", "bf16"):
            route = (C.c_int32 * 2)(0, 0)

            def call():
                if name == "fp32":
                    return lib.dsg_debug_t_gemm(1, 0, p(dy), out_, p(xx), in_, None, p(dW), in_, out_, in_, rows, 0, p(db), None, 0, None, 0, route, None)
                return lib.dsg_debug_t_gemm_lp(1, 0, p(dy), out_, p(xx), in_, None, p(dW), in_, out_, in_, rows, 0, p(db), None, 0, None, 0, route, None)
            for _ in range(3):
                assert call() == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(rep):
                call()
            e1.record(); torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / rep
            res[name + "_ms"], res[name + "_tflops"], res[name + "_route"], res[name + "_slices"] = ms, res["flop"] / ms / 1e9, route[0], route[1]
        print("TBJSON " + json.dumps(res), flush=True)


def run_child(tree, mode, limit):
    """a fresh process of `tree`'s copy of this tool (the parent's tree has none: this file is run with ROOT pointed at it)"""
    env = dict(os.environ, TB_ROOT=tree)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child {mode} of {tree} ended with status {r.returncode}: stopping")   # nothing more is started on the GPU
    rows = [json.loads(l[len("TBJSON "):]) for l in r.stdout.splitlines() if l.startswith("TBJSON ")]
    return rows


def main():
    global ROOT
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--child", choices=["fp32", "bf16", "parent", "kernels"])
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.child:
        ROOT = os.environ.get("TB_ROOT", ROOT)
        if args.child == "kernels":
            child_kernels()
        else:
            child_iterations(None if args.child == "parent" else args.child)
        return
    if not args.parent:
        ap.error("--parent DIR (a built checkout of the parent commit) or --child MODE")
    runs = {"parent": [], "fp32": [], "bf16": []}
    for r in range(args.rounds):
        order = [("parent", os.path.abspath(args.parent), "parent"), ("fp32", ROOT, "fp32"), ("bf16", ROOT, "bf16")]
        for tag, tree, mode in order[r % 3:] + order[:r % 3]:   # rotated: no build always runs behind the same predecessor
            row = run_child(tree, mode, 400)[0]
            row["run"], row["round"] = tag, r
            runs[tag].append(row)
            print("TBJSON " + json.dumps(row), flush=True)
    for row in run_child(ROOT, "kernels", 300):
        print("TBJSON " + json.dumps(row), flush=True)
    for key in ("no_sc_mean_s", "sc_mean_s"):
        v = {tag: [x[key] for x in rows] for tag, rows in runs.items()}
        spread = max(v["parent"]) - min(v["parent"])
        med = {tag: sorted(xs)[len(xs) // 2] for tag, xs in v.items()}
        print(f"TBSUM {key}: parent {v['parent']} (spread {spread:.5f}), fp32 {v['fp32']}, bf16 {v['bf16']}; medians parent {med['parent']:.5f} "
              f"fp32 {med['fp32']:.5f} bf16 {med['bf16']:.5f}; fp32 inside the parent's spread: {min(v['parent']) - spread <= med['fp32'] <= max(v['parent']) + spread}; "
              f"bf16 faster than the parent by more than its spread: {med['parent'] - med['bf16'] > spread} (ratio {med['parent'] / med['bf16']:.3f})", flush=True)


if __name__ == "__main__":
    main()
