"""GPU: the bf16 mode of the training entries (dsg_train_set_precision; train.py's precision="bf16") end to end, against
tests/golden/train_bf16.npz -- the reference's own modules with the mode's arithmetic emulated in-process (tools/gen_train_bf16_golden.py:
the covered linears round both operands of their three products to bf16 and multiply in float64).

Bars, all from the fixture and the issue, none from the library's output: the loss within 2e-4; every parameter gradient within
2e-4 + 4 d_flip of its tensor's scale, d_flip the fixture's measured sensitivity of the emulation to rounding decisions that flip under
last-bit input differences (one draw of a heavy-tailed quantity, hence the factor 4).  The same bar must be VIOLATED by fp32 mode on a
covered weight tensor of each case -- a build that ignores the switch fails there.

The fixture's own non-vacuity condition (every covered weight with e_bf16 > 1e-3 has 2e-4 + 4 d_flip <= e_bf16 / 4) does NOT hold
for these networks: with the portable generator's weights the emulation itself moves by d_flip = 1e-3 ... 1.3e-2 under a 2^-22 input
perturbation.  small_b8: 26 of 27 covered weights satisfy it (down_layers.1.blocks.0.mlp.fc2: 3.7e-2 against 1.75e-2); tiny_b8: none of
9 (e_bf16 4.9e-3 ... 9.9e-3, 4 d_flip 2.9e-3 ... 1.2e-2).  B = 16 and a 2^-23 perturbation, the two remedies tried, change neither
count.  The tool writes the fixture and then fails on that assertion; the checks below are the issue's, unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W
from util import load

pytestmark = pytest.mark.gpu

CASES = list(Y.TRAIN_BF16_CASES)
_nets = {}


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _fresh_net(cfg_name):
    from diffusesg_amd.model import build_network
    cfg = Y.CONFIGS[cfg_name]()
    return build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")


def _net(cfg_name):
    if cfg_name not in _nets:
        _nets[cfg_name] = _fresh_net(cfg_name)
    return _nets[cfg_name]


def _step(case, precision, results={}):
    """one dsg_train_step_grads of the case in `precision` -> (loss, {key: flat gradient}, route counts); computed once per (case, mode)"""
    if (case, precision) in results:
        return results[case, precision]
    from diffusesg_amd.train import NodeAdjEDMObjectiveGeneratorHip, NodeAdjRainbowLossHip, train_step_grads
    cfg, flags, clean_adj, clean_node, rnd, eps_adj, eps_node, coin, _ = Y.train_bf16_case(case)
    model = _net(Y.TRAIN_BF16_CASES[case][0])
    gen = NodeAdjEDMObjectiveGeneratorHip(precond="edm", sigma_dist="edm", other_params=None, dev="cuda", symmetric_noise=False)
    loss_func = NodeAdjRainbowLossHip(edge_loss_weight=1.0, node_loss_weight=1.0, flag_reweight=False, objective="edm")
    na, nx, cond, ta, tx, (c_skip, c_out, c_in, c_noise, sigmas, weights) = gen.get_input_output(
        T(clean_adj), T(clean_node), T(flags), rnd_sigma=T(rnd), noise=(T(eps_adj), T(eps_node)))
    real = np.random.rand
    np.random.rand = lambda: coin
    try:
        oa, on, la, ln, grads = train_step_grads(model, loss_func, na, nx, T(flags), sigmas, T(clean_adj), T(clean_node), weights,
                                                 iou_loss_weight=1.0, precision=precision)
    finally:
        np.random.rand = real
    h = model.model._ensure_handle()
    assert h.get_train_precision() == "fp32", "the call must restore the handle's mode"
    out = (float(la.mean() + ln.mean()), {k: v.cpu().numpy().reshape(-1) for k, v in grads.items()}, h.train_routes())
    results[case, precision] = out
    return out


def _errors(case, grads):
    """per tensor: (key, max |mine - E| over the stored sample / max |E|, the bar 2e-4 + 4 d_flip, covered)"""
    g = load("train_bf16.npz")
    names = [str(k) for k in g[f"{case}_gparam_names"]]
    assert set(k[len("model."):] for k in names) == set(grads)
    rows = []
    for i, k in enumerate(names):
        mine, ref = grads[k[len("model."):]], g[f"{case}_gparam/{k}"]
        stride = max(1, -(-mine.size // Y.TRAIN_BF16_MAX_SAMPLE))
        err = float(np.abs(mine[::stride] - ref).max()) / max(float(np.abs(ref).max()), 1e-30)
        rows.append((k, err, 2e-4 + 4.0 * float(g[f"{case}_d_flip"][i]), bool(g[f"{case}_covered"][i])))
    return rows


@pytest.mark.parametrize("case", CASES)
def test_bf16_mode_matches_the_emulation(case):
    g = load("train_bf16.npz")
    loss, grads, _ = _step(case, "bf16")
    ref_loss = float(g[f"{case}_loss"])
    rows = _errors(case, grads)
    worst = max(rows, key=lambda r: r[1] / r[2])
    print(f"TRAINBF16 {case} bf16 vs E: loss {loss:.6f} (E {ref_loss:.6f}, rel {abs(loss - ref_loss) / abs(ref_loss):.2e}); worst tensor "
          f"{worst[0]} err {worst[1]:.2e} bar {worst[2]:.2e}; tensors above their bar: {sum(r[1] > r[2] for r in rows)} of {len(rows)}")
    assert abs(loss - ref_loss) <= 2e-4 * abs(ref_loss)
    bad = [(k, f"{e:.2e}", f"{b:.2e}") for k, e, b, _ in rows if e > b]
    assert not bad, bad


@pytest.mark.parametrize("case", CASES)
def test_fp32_mode_violates_the_same_bar(case):
    """power: on the same inputs fp32 mode is outside 2e-4 + 4 d_flip of (E) on at least one covered weight tensor"""
    _, grads, routes = _step(case, "fp32")
    assert routes == {}, "fp32 mode lists no covered product"
    rows = [r for r in _errors(case, grads) if r[3]]
    out = [r for r in rows if r[1] > r[2]]
    print(f"TRAINBF16 {case} fp32 vs E: {len(out)} of {len(rows)} covered weights outside their bar; largest err / bar "
          f"{max(r[1] / r[2] for r in rows):.2f}")
    assert out, "fp32 mode sits inside the bf16 bars on every covered weight: the bars cannot tell the modes apart"


def _expected_routes(case):
    """{(rows, class): (bf16, fp32)} of one dsg_train_step_grads: per level 4 products per block (encoder and decoder blocks), the
    merging into the level, the breakup's pre_linear out of it and its post_linear into it -- each once as y, dx and dW"""
    cfg_name, B, _, _ = Y.TRAIN_BF16_CASES[case]
    cfg = Y.CONFIGS[cfg_name]()
    L = len(cfg.depths)
    want = {}
    for l in range(L):
        rows = B * (cfg.max_node_num >> l) ** 2
        n = 4 * 2 * cfg.depths[l] + (1 if l >= 1 else 0) + (1 if l >= 1 else 0) + (1 if l <= L - 2 else 0)
        for cls in range(3):
            want[rows, cls] = (n, 0) if rows >= 512 else (0, n)
    return want


@pytest.mark.parametrize("case", CASES)
def test_route_counts(case):
    """every covered product of a level with >= 512 rows on the bf16 route, tiny's level 1 (128 rows) on none, and nothing else listed:
    PatchEmbed, the read-out chain and the heads share level 0's row count and would show up as extra products there"""
    _, _, routes = _step(case, "bf16")
    want = _expected_routes(case)
    assert routes == want, (routes, want)
    if case == "tiny_b8":
        assert want[512, 0] == (9, 0) and want[128, 2] == (0, 10)
    else:
        assert want[2048, 2] == (17, 0) and want[512, 1] == (10, 0)


def _train_grads(model, name, B):
    """dsg_train_grads with a seeded dL/dF -> {"F_adj", "F_node", every parameter's gradient by key} as CPU tensors"""
    from diffusesg_amd import train as TR
    cfg, flags, ca, cn, rnd, _ea, _en, _coin = Y.train_case(name, B=B)
    m = model.model
    h = TR._train_handle(m)
    n = cfg.max_node_num
    ia, ix, c_noise, fl = T(ca), T(cn), T((0.25 * rnd).astype(np.float32)), T(flags.astype(np.uint8))
    dFa, dFn = T(W.normal(5, "lp/dF_adj", (B, cfg.c_adj, n, n))), T(W.normal(5, "lp/dF_node", (B, n, cfg.c_node)))
    Fa, Fn = torch.empty_like(ia), torch.empty_like(ix)
    keys, offs, shapes, total = TR._flat_layout(m)
    flat = torch.zeros(total, device="cuda")
    names = (C.c_char_p * len(keys))(*[k.encode() for k in keys])
    ptrs = (C.c_void_p * len(keys))(*[flat.data_ptr() + 4 * o for o in offs])
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h.check(h.L.dsg_train_grads(h.raw, B, p(ia), p(ix), p(fl), p(c_noise), None, None, p(dFa), p(dFn), p(Fa), p(Fn), len(keys), names, ptrs, st),
            "dsg_train_grads")
    flat = flat.cpu()
    out = {"F_adj": Fa.cpu(), "F_node": Fn.cpu()}
    out.update({k: flat[o:o + int(np.prod(s))].clone() for k, o, s in zip(keys, offs, shapes)})
    return out


def _same_bits(a, b, noise):
    """every tensor torch.equal -- with the one exception tests/test_workspace_poison.py documents for the fp32 training form: the
    gradients of the relative-position bias tables are accumulated by the attention backward with float atomics in no fixed order, so
    two runs of the SAME code already differ in their last bits.  They are held to that file's bar: 8 x max(the difference of two
    runs before the switch was ever touched, 2^-20 of the tensor's maximum)."""
    bad = []
    for k in a:
        if k.endswith("relative_position_bias_table"):
            bar = 8.0 * max(noise[k], 2.0 ** -20 * float(a[k].abs().max()))
            if float((a[k] - b[k]).abs().max()) > bar:
                bad.append(k)
        elif not torch.equal(a[k], b[k]):
            bad.append(k)
    return bad


def test_neutrality_of_the_switch():
    """dsg_train_grads on a handle that never saw the switch, after setting mode 1, and after setting it back to 0.  B = 4 (256 / 64
    rows: no product takes the route, so mode 1 is the same bits too); B = 8 (512 rows at level 0): mode 1 differs, mode 0 afterwards
    is bit for bit what it was (bias-table gradients: see _same_bits).  Bad mode values return DSG_ERR_INVALID and keep the mode."""
    from diffusesg_amd import lib as L
    model = _fresh_net("tiny")
    first = {B: _train_grads(model, "tiny", B) for B in (4, 8)}
    noise = {}
    for B in (4, 8):   # run-to-run difference of the atomically accumulated bias-table gradients, before the switch is touched
        rerun = _train_grads(model, "tiny", B)
        noise[B] = {k: float((first[B][k] - rerun[k]).abs().max()) for k in rerun if k.endswith("relative_position_bias_table")}
        assert _same_bits(first[B], rerun, noise[B]) == []
    h = model.model._ensure_handle()
    assert h.get_train_precision() == "fp32"
    h.set_train_precision("bf16")
    assert h.get_train_precision() == "bf16"
    for bad in (2, -1, 7):
        assert h.L.dsg_train_set_precision(h.raw, bad) == L.DSG_ERR_INVALID
        assert h.get_train_precision() == "bf16"
    on4, on8 = _train_grads(model, "tiny", 4), _train_grads(model, "tiny", 8)
    assert _same_bits(first[4], on4, noise[4]) == [], "below the shape rule mode 1 must stay on the fp32 routes"
    assert h.train_routes() and all(v[0] > 0 for (rows, _), v in h.train_routes().items() if rows == 512)
    assert not torch.equal(first[8]["down_layers.0.blocks.0.mlp.fc1.weight"], on8["down_layers.0.blocks.0.mlp.fc1.weight"]), "mode 1 changed nothing at 512 rows"
    h.set_train_precision("fp32")
    for B in (4, 8):
        again = _train_grads(model, "tiny", B)
        assert _same_bits(first[B], again, noise[B]) == [], f"B = {B}: mode 0 after mode 1 is not the bits it was"
    assert h.train_routes() == {}
    with pytest.raises(ValueError):
        h.set_train_precision("fp16")


def test_fp32_entries_ignore_the_mode():
    """dsg_precond_vjp and a short dsg_ode_run with a probe: bit-equal with the mode at 1 and at 0 (B = 8: 512 rows at level 0)"""
    from diffusesg_amd import ode
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg, flags, clean_adj, clean_node, rnd, eps_adj, eps_node, _, _ = Y.train_bf16_case("tiny_b8")
    model = _net("tiny")
    h = model.model._ensure_handle()
    B = flags.shape[0]
    adj, node = T(W.mask_adj(clean_adj + 0.5 * eps_adj, flags)), T(W.mask_node(clean_node + 0.5 * eps_node, flags))
    sig = T(np.full(B, 0.7, np.float32))
    ga, gn = T(W.normal(9, "lp/vjp_adj", clean_adj.shape)), T(W.normal(9, "lp/vjp_node", clean_node.shape))
    smp = NodeAdjEDMSamplerHip(num_steps=3, solver="euler", S_churn=0.0, dev="cuda", objective="edm", self_condition=True, symmetric_noise=False)
    seeds = np.arange(1, B + 1, dtype=np.uint64)
    res = {}
    try:
        for mode in ("bf16", "fp32"):
            h.set_train_precision(mode)
            vj = model.value_and_input_grad(adj, node, T(flags), sig, grad_outputs=(ga, gn), coin=False)
            od = ode.run(model, smp, adj, node, T(flags), "encode", "rademacher", graph_seeds=seeds)
            res[mode] = [t.cpu() for t in vj if torch.is_tensor(t)] + [od[0].cpu(), od[1].cpu(), od[2].cpu()]
    finally:
        h.set_train_precision("fp32")
    assert len(res["bf16"]) >= 6
    for a, b in zip(res["bf16"], res["fp32"]):
        assert torch.equal(a, b)


def test_patch_handle_accepts_the_setter_and_still_refuses_training():
    from diffusesg_amd import lib as L
    from diffusesg_amd.model import build_network
    cfg = Y.PATCH_CONFIGS["tiny_p2"]()
    h = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda").model._ensure_handle()
    h.set_train_precision("bf16")
    assert h.get_train_precision() == "bf16"
    assert h.L.dsg_train_grads(h.raw, 2, *([None] * 10), 0, None, None, None) == L.DSG_ERR_INVALID
    assert "patch_size" in h.L.dsg_last_error(h.raw).decode()
    assert h.L.dsg_train_self_cond(h.raw, 2, *([None] * 7)) == L.DSG_ERR_INVALID
    assert "patch_size" in h.L.dsg_last_error(h.raw).decode()


def test_one_iteration_in_bf16_mode():
    """train_one_iteration(precision="bf16") with AdamHip and one EMAHip: parameters and both moments stay fp32 and finite, the returned
    gradient norm is within 1e-4 + 4 max d_flip of (E)'s, the handle's mode is back at fp32"""
    from diffusesg_amd.train import AdamHip, EMAHip, NodeAdjEDMObjectiveGeneratorHip, NodeAdjRainbowLossHip, train_one_iteration
    g = load("train_bf16.npz")
    case = "tiny_b8"
    cfg, flags, clean_adj, clean_node, rnd, eps_adj, eps_node, coin, _ = Y.train_bf16_case(case)
    model = _fresh_net("tiny")
    gen = NodeAdjEDMObjectiveGeneratorHip(precond="edm", sigma_dist="edm", other_params=None, dev="cuda", symmetric_noise=False)
    loss_func = NodeAdjRainbowLossHip(edge_loss_weight=1.0, node_loss_weight=1.0, flag_reweight=False, objective="edm")
    opt = AdamHip(model, lr=2.0e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    emas = [EMAHip(model, beta=0.9999)]
    real = np.random.rand
    np.random.rand = lambda: coin
    try:
        loss, ra, rn, sg, total_norm = train_one_iteration(model, gen, loss_func, opt, emas, T(clean_adj), T(clean_node), T(flags),
                                                           iou_loss_weight=1.0, precision="bf16", rnd_sigma=T(rnd), noise=(T(eps_adj), T(eps_node)))
    finally:
        np.random.rand = real
    h = model.model._ensure_handle()
    assert h.get_train_precision() == "fp32"
    assert any(v[0] > 0 for v in h.train_routes().values()), "the iteration did not run in bf16 mode"
    for group in (opt.params, opt.exp_avg, opt.exp_avg_sq, list(emas[0].shadow.values())):
        for t in group:
            assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
    ref = float(g[f"{case}_total_grad_norm"])
    bar = 1e-4 + 4.0 * float(g[f"{case}_d_flip"].max())
    print(f"TRAINBF16 {case} iteration: |grad| {total_norm:.5f} (E {ref:.5f}, rel {abs(total_norm - ref) / ref:.2e}, bar {bar:.2e}), loss {float(loss):.6f}")
    assert abs(total_norm - ref) <= bar * ref
    assert abs(float(loss) - float(g[f"{case}_loss"])) <= 2e-4 * abs(float(g[f"{case}_loss"]))
