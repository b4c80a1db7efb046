"""Training-mode BatchNorm3d of stage 0 under hip_grad() on the GPU (csrc/batchnorm.hip, the Columns layout,
stage0_grad.BatchNorm3dActFunction, CostRegNetNoDown in .train() mode) against the float64 restatements of
tests/_stage0_bn_train_ref.py:
  1. decnet_bn_train_cl_forward / _backward through the C ABI on channels-last matrices [rows, C] at the edge shapes, at
     both placements and under both LDS poison words (tests/_placement._both), every bound counted from roundings
     (u = 2^-24; _bn_train_ref.check_entry): the bounds tests/test_bn_train_gpu.py holds the 2-D entries to;
  2. the recomputed ReLU decision, gz left out, a NaN planted in one channel, a constant channel, bit-identical repeats and
     graph replays, refusals that launch nothing;
  3. BatchNorm3dActFunction behind Conv3dFunction on single units;
  4. CostRegNetNoDown.stage0 in .train() mode: entries taken, every gradient against the float64 train-mode run with the
     GPU's masks imposed, running statistics after 1 and 3 steps, the caches that fold them, frozen units inside a
     training module, a GraphedStep, and the refusals.
-m gpu."""
import copy
import math

import pytest
import torch

import _bn_train_ref as BR
import _model_cases as MC
import _stage0_bn_train_ref as SB
import _stage0_grad_ref as SG
from _placement import ERR_MISALIGNED, Place, _L, _bits_equal, _both, _st
from test_stage0_edges_gpu import TOL_WINO

pytestmark = pytest.mark.gpu
ERR_NULL, ERR_SHAPE = -1, -2
EPS, MOM = 1e-5, 0.1
CASES = SB.entry_cases()
IDS = ["%dx%d" % c for c in CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from decnet_amd import ops2d
    assert ops2d.BN_CL_ROWS == SB.ROWS
    return torch.device("cuda:0")


# ---- 1. the entries -----------------------------------------------------------------------------------------------------------
def _ws(L, dev, rows, C):
    n = L.decnet_bn_train_cl_workspace_floats(rows, C)
    assert n == 2 * (2 * -(-rows // SB.ROWS) * C + 2 * C), (rows, C, n)
    return torch.full((n,), float("nan"), dtype=torch.float32, device=dev), n        # torch allocations: 16-byte aligned


def _run_entry(rows, C, first_kind, relu, ones=False, want_gz=True, aligned=True):
    """Forward, then backward on the forward's stats, through the C ABI on the channels-last matrices -> the results on the
    CPU, y and gz in the [1, C, 1, rows] view of the reference."""
    L, dev = _L(), torch.device("cuda:0")
    d = SB.entry_data(rows, C, first_kind, relu)
    gy = torch.ones(rows, C) if ones else SB.to_cl(d["gy"])
    P = Place(dev, aligned)
    z, gyd, gamma, beta = P.inp(SB.to_cl(d["z"])), P.inp(gy), P.inp(d["gamma"]), P.inp(d["beta"])
    rm, rv = P.inplace(d["running_mean"]), P.inplace(d["running_var"])
    stats, y = P.out((2 * C,), torch.float64), P.out((rows, C))
    gz = P.out((rows, C)) if want_gz else None
    dg, db = P.out((C,)), P.out((C,))
    ws, nws = _ws(L, dev, rows, C)                              # NaN-filled: nothing of it may come out
    rc = L.decnet_bn_train_cl_forward(z.data_ptr(), gamma.data_ptr(), beta.data_ptr(), EPS, MOM, rm.data_ptr(),
                                      rv.data_ptr(), stats.data_ptr(), y.data_ptr(), int(relu), ws.data_ptr(), nws, rows, C,
                                      _st())
    assert rc == 0, rc
    ws2, _ = _ws(L, dev, rows, C)                               # (a fresh one: the backward reads nothing the forward left)
    rc = L.decnet_bn_train_cl_backward(z.data_ptr(), gyd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), stats.data_ptr(),
                                       gz.data_ptr() if want_gz else None, dg.data_ptr(), db.data_ptr(), int(relu),
                                       ws2.data_ptr(), nws, rows, C, _st())
    assert rc == 0, rc
    P.check("bn_train_cl %s" % ((rows, C),))
    assert not bool(torch.isnan(stats).any())
    out = {"y": SB.from_cl(y.cpu()), "stats": stats.cpu(), "running_mean": rm.cpu(), "running_var": rv.cpu(),
           "dgamma": dg.cpu(), "dbeta": db.cpu()}
    if want_gz:
        out["gz"] = SB.from_cl(gz.cpu())
    return out


_REFS = {}


def _ref(rows, C, first_kind, relu):
    """The float64 forward of a case, computed once."""
    key = (rows, C, first_kind, relu)
    if key not in _REFS:
        d = SB.entry_data(rows, C, first_kind, relu)
        _REFS[key] = (d, BR.forward(d["z"], d["gamma"], d["beta"], EPS, MOM, d["running_mean"], d["running_var"], relu))
    return _REFS[key]


@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("first_kind", [0, 1, 2], ids=BR.KINDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_entries_against_float64(dev, case, first_kind, relu):
    rows, C = case
    r = _both(_run_entry, rows, C, first_kind, relu)
    d, f = _ref(rows, C, first_kind, relu)
    BR.check_entry(r, f, d["gamma"], d["beta"], d["gy"], relu, EPS, (case, first_kind, relu))
    if relu and C > 1:                                          # the channel with every pre-activation below zero
        c = C - 1
        assert not bool(r["y"][:, c].any()) and not bool(r["gz"][:, c].any())
        assert float(r["dgamma"][c]) == 0.0 and float(r["dbeta"][c]) == 0.0
    for c in range(C):                                          # a constant channel: var = 0 exactly
        if BR.KINDS[(c + first_kind) % 3] == "constant":
            want = 1.0 / math.sqrt(EPS)
            assert abs(float(r["stats"][2 * c + 1]) - want) <= 4 * 2.0 ** -53 * want, (case, c)
            assert float(r["stats"][2 * c]) == float(d["z"][0, c, 0, 0])


# ---- 2. decisions, NaNs, determinism, refusals ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES[1:], ids=IDS[1:])
def test_backward_recomputes_the_forward_relu_decision(dev, case):
    """gy = 1: dbeta[c] is the number of elements the backward let through, and equals the count of y[:, c] > 0 exactly."""
    for first_kind in (0, 1):
        for aligned in (True, False):
            r = _run_entry(*case, first_kind, True, ones=True, aligned=aligned)
            assert torch.equal(r["dbeta"], (r["y"] > 0).sum((0, 2, 3)).float()), (case, first_kind, aligned)


def test_parameter_gradients_alone(dev):
    """gz NULL: two launches, the same dgamma and dbeta."""
    case = (SB.ROWS + 1, 5)
    a, b = _run_entry(*case, 0, True), _run_entry(*case, 0, True, want_gz=False)
    assert "gz" not in b and all(_bits_equal(a[k], b[k]) for k in b)


@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
def test_a_nan_stays_in_its_channel(dev, relu):
    from decnet_amd import ops2d
    rows, C, bad = 3 * SB.ROWS + 1, 20, 7                       # (20 channels: two finish workgroups, `bad` in the first)
    d = SB.entry_data(rows, C, 0, False)
    t = {k: v.to(dev) for k, v in d.items()}
    z, gy = SB.to_cl(d["z"]), SB.to_cl(d["gy"]).to(dev)
    z[2 * SB.ROWS + 3, bad] = float("nan")
    z = z.to(dev)
    rm, rv = t["running_mean"].clone(), t["running_var"].clone()
    y, stats = ops2d.bn_train_cl_forward(z, t["gamma"], t["beta"], EPS, MOM, rm, rv, relu)
    gz, dg, db = ops2d.bn_train_cl_backward(z, gy, t["gamma"], t["beta"], stats, relu)
    other = [c for c in range(C) if c != bad]
    for name, v in (("y", y), ("gz", gz)):
        assert bool(torch.isnan(v[:, bad]).all()), name
        assert not bool(torch.isnan(v[:, other]).any()), name
    for name, v in (("mean", stats[0::2]), ("invstd", stats[1::2]), ("running_mean", rm), ("running_var", rv), ("dgamma", dg)):
        assert bool(torch.isnan(v[bad])), name
        assert not bool(torch.isnan(v[other]).any()), name
    # (dbeta = sum gm holds no z: without ReLU it is the sum of gy, with ReLU the NaN element's decision pre > 0 is false)
    assert not bool(torch.isnan(db).any())


def _graph_run(dev, run, reset):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for _ in range(2):
        reset()
        for v in out.values():
            v.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        yield {k: v.cpu() for k, v in out.items()}


def test_two_calls_and_graph_replays_are_bit_identical(dev):
    """(The aligned and the unaligned placement have the same bits as each other in every case of
    test_entries_against_float64: `_both` requires it.)"""
    from decnet_amd import ops2d
    rows, C = 5 * SB.ROWS + 1, 216
    first = _run_entry(rows, C, 1, True)
    again = _run_entry(rows, C, 1, True)
    for k in first:
        assert _bits_equal(first[k], again[k]), k
    d = SB.entry_data(rows, C, 1, True)
    t = {k: v.to(dev) for k, v in d.items()}
    z, gy = SB.to_cl(d["z"]).to(dev), SB.to_cl(d["gy"]).to(dev)
    rm, rv = t["running_mean"].clone(), t["running_var"].clone()

    def run():
        y, stats = ops2d.bn_train_cl_forward(z, t["gamma"], t["beta"], EPS, MOM, rm, rv, True)
        gz, dg, db = ops2d.bn_train_cl_backward(z, gy, t["gamma"], t["beta"], stats, True)
        return {"y": y, "stats": stats, "gz": gz, "dgamma": dg, "dbeta": db}

    def reset():
        rm.copy_(t["running_mean"])
        rv.copy_(t["running_var"])

    for got in _graph_run(dev, run, reset):
        got.update(running_mean=rm.cpu(), running_var=rv.cpu(), y=SB.from_cl(got["y"]), gz=SB.from_cl(got["gz"]))
        for k in first:
            assert _bits_equal(first[k], got[k]), "%s differs between the eager call and a graph replay" % k


def test_rejections_launch_nothing(dev):
    L = _L()
    rows, C = 70, 3
    d = SB.entry_data(rows, C, 0, True)
    P = Place(dev, True)
    z, gy, gamma, beta = P.inp(SB.to_cl(d["z"])), P.inp(SB.to_cl(d["gy"])), P.inp(d["gamma"]), P.inp(d["beta"])
    rm, rv = P.inp(d["running_mean"]), P.inp(d["running_var"])
    stats, y, gz, dg, db = P.out((2 * C,), torch.float64), P.out((rows, C)), P.out((rows, C)), P.out((C,)), P.out((C,))
    ws, nws = _ws(L, dev, rows, C)
    big = torch.full((nws + 8,), float("nan"), dtype=torch.float32, device=dev)
    odd = torch.full((4 * C + 4,), float("nan"), dtype=torch.float32, device=dev)[1:]           # a stats off by 4 bytes
    assert odd.data_ptr() % 8 == 4

    def fwd(z_=z.data_ptr(), rm_=rm.data_ptr(), rv_=rv.data_ptr(), stats_=stats.data_ptr(), ws_=ws.data_ptr(), n_=nws,
            dims=(rows, C)):
        return L.decnet_bn_train_cl_forward(z_, gamma.data_ptr(), beta.data_ptr(), EPS, MOM, rm_, rv_, stats_, y.data_ptr(), 1,
                                            ws_, n_, *dims, _st())

    def bwd(gy_=gy.data_ptr(), stats_=stats.data_ptr(), dg_=dg.data_ptr(), ws_=ws.data_ptr(), n_=nws, dims=(rows, C)):
        return L.decnet_bn_train_cl_backward(z.data_ptr(), gy_, gamma.data_ptr(), beta.data_ptr(), stats_, gz.data_ptr(), dg_,
                                             db.data_ptr(), 1, ws_, n_, *dims, _st())

    assert fwd(z_=None) == ERR_NULL and fwd(stats_=None) == ERR_NULL and bwd(gy_=None) == ERR_NULL and bwd(dg_=None) == ERR_NULL
    assert fwd(dims=(1, C)) == ERR_SHAPE and bwd(dims=(1, C)) == ERR_SHAPE                       # rows = 1
    assert fwd(dims=(rows, 0)) == ERR_SHAPE and bwd(dims=(rows, 0)) == ERR_SHAPE                 # C = 0
    assert fwd(n_=nws - 1) == ERR_SHAPE and bwd(n_=nws - 1) == ERR_SHAPE                         # a short workspace
    assert fwd(ws_=big.data_ptr() + 4, n_=nws + 4) == ERR_MISALIGNED                             # off by 4 bytes
    assert bwd(ws_=big.data_ptr() + 4, n_=nws + 4) == ERR_MISALIGNED
    assert fwd(stats_=odd.data_ptr()) == ERR_MISALIGNED and bwd(stats_=odd.data_ptr()) == ERR_MISALIGNED
    assert fwd(rm_=None) == ERR_NULL and fwd(rv_=None) == ERR_NULL                               # one of the two alone
    assert fwd(ws_=None) == ERR_NULL and bwd(ws_=None) == ERR_NULL
    P.check_untouched("rejected bn_train_cl")
    assert bool(torch.isnan(ws).all()) and bool(torch.isnan(big).all()) and bool(torch.isnan(odd).all())
    assert fwd(rm_=None, rv_=None) == 0 and bwd() == 0          # without running statistics; and the complete backward
    P.check("accepted bn_train_cl")


# ---- 3. BatchNorm3dActFunction behind Conv3dFunction on one unit ---------------------------------------------------------------
UNITS = {"8to8": (8, 8, True), "8to1_norelu": (8, 1, False), "216to216": (216, 216, True)}      # name: (Ci, Co, relu)
DIMS = (2, 3, 4, 5)


def _graph_names(t):
    seen, names, todo = set(), [], [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        todo.extend(f for f, _ in fn.next_functions)
    return names


def _library_nodes(names):
    return [n for n in names if ("Convolution" in n or "BatchNorm" in n) and not n.startswith("BatchNorm3dActFunction")]


@pytest.mark.parametrize("name", sorted(UNITS))
def test_function_on_units(dev, name):
    from decnet_amd import BatchNorm3dActFunction, Conv3dFunction, stage0, stage0_grad
    Ci, Co, relu = UNITS[name]
    B, D, H, W = DIMS
    rows = B * D * H * W
    g = torch.Generator().manual_seed(Ci * 5 + Co)
    x = torch.randn(*DIMS, Ci, generator=g)
    w = torch.randn(Co, Ci, 3, 3, 3, generator=g) / (27 * Ci) ** 0.5
    gamma, beta = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.3
    gamma[::2] = -gamma[::2]
    rm, rv = torch.randn(Co, generator=g) * 0.2, torch.rand(Co, generator=g) + 0.5
    gy = torch.randn(*DIMS, Co, generator=g)
    xd, wd, gd, bd = (t.to(dev).requires_grad_() for t in (x, w, gamma, beta))
    rmd, rvd = rm.to(dev), rv.to(dev)
    versions = (rmd._version, rvd._version)
    packed = stage0_grad.unit_operands(wd.detach(), stage0.WINO_VARIANT.get(stage0.conv_algo(D)), last=(Co == 1))
    z = Conv3dFunction.apply(packed, False, wd, torch.ones(Co, device=dev), torch.zeros(Co, device=dev), xd)
    z.retain_grad()
    y = BatchNorm3dActFunction.apply(z, gd, bd, rmd, rvd, EPS, MOM, relu)
    names = _graph_names(y)
    assert "BatchNorm3dActFunctionBackward" in names and "Conv3dFunctionBackward" in names, names
    assert not _library_nodes(names), names
    assert rmd._version > versions[0] and rvd._version > versions[1]
    y.backward(gy.to(dev))
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in (xd, wd))
    # float64 on the GPU's own z
    zc = z.detach().cpu().reshape(rows, Co)
    f = SB.forward(zc, gamma, beta, EPS, MOM, rm, rv, relu)
    stats = torch.stack((f["mean"], f["invstd"]), 1).reshape(-1)          # (the Function keeps its stats: held through y)
    r = {"y": SB.from_cl(y.detach().cpu().reshape(rows, Co)), "stats": stats, "running_mean": rmd.cpu(), "running_var": rvd.cpu(),
         "gz": SB.from_cl(z.grad.cpu().reshape(rows, Co)), "dgamma": gd.grad.cpu(), "dbeta": bd.grad.cpu()}
    BR.check_entry(r, f, gamma, beta, SB.from_cl(gy.reshape(rows, Co)), relu, EPS, name)


# ---- 4. the module in .train() mode -------------------------------------------------------------------------------------------
def _leaves(mod, L, R):
    return {"L": L, "R": R, **dict(mod.named_parameters())}


def _gpu_step(mod, L, R, D, r, r2):
    """(pred r).sum() + (reg r2).sum() through mod.stage0 under hip_grad() -> (pred, reg, [y_i of every unit], entries)."""
    import decnet_amd
    from spy_util import entry_spy
    rec, orig = {}, mod._units_grad

    def spy(x):
        rec["outs"] = orig(x)
        return rec["outs"]
    mod._units_grad = spy
    try:
        with entry_spy() as calls:
            with decnet_amd.hip_grad():
                pred, reg = mod.stage0(L, R, D, return_reg=True)
            ((pred * r).sum() + (reg * r2).sum()).backward()
            torch.cuda.synchronize()
    finally:
        del mod._units_grad
    return pred, reg, [o.detach() for o in rec["outs"]], list(calls)


def _on_gpu(name, dev, frozen=()):
    mod, L, R, D, r, r2 = SG.module_case(name)
    modg = copy.deepcopy(mod).to(dev).train()
    for i in frozen:
        modg.units()[i].bn.eval()
    Lg, Rg = (t.to(dev).requires_grad_() for t in (L, R))
    return mod, modg, (L, R, D, r, r2), (Lg, Rg, D, r.to(dev), r2.to(dev))


def _masks_of(outs, mod):
    return [(o > 0).permute(0, 4, 1, 2, 3).cpu() if u.relu else None for o, u in zip(outs, mod.units())]


def _clear(modg, Lg, Rg):
    for p in _leaves(modg, Lg, Rg).values():
        p.grad = None


_PARITY = {}


def parity_ratios(name):
    """One train-mode step of case `name` on the GPU, then two more; the float64 and float32 CPU runs with the GPU's masks
    imposed -> the rows tools/bench_stage0_bn_train.py --parity writes to profiles/stage0_bn_train_parity.json, and what
    test_module_against_float64 asserts on.  The gate is tests/test_stage0_grad_gpu._check_grads's:
    max(4 max|g32 - g64|, 2e-5 max(1, max|g64|)), g32 the float32 CPU run under the same masks.  Computed once per case."""
    if name in _PARITY:
        return _PARITY[name]
    dev = torch.device("cuda:0")
    mod, modg, cpu, gpu = _on_gpu(name, dev)
    Lg, Rg, D = gpu[:3]
    stats = [(u.bn.running_mean, u.bn.running_var) for u in modg.units()]
    versions = [(m._version, v._version) for m, v in stats]
    with torch.no_grad():
        pred_old = copy.deepcopy(modg).eval().stage0(Lg, Rg, D)
    pred, reg, outs, calls = _gpu_step(modg, *gpu)
    names = _graph_names(pred)
    got = {k: t.grad.detach().cpu() for k, t in _leaves(modg, Lg, Rg).items()}
    bufs = [{k: b.detach().cpu().clone() for k, b in modg.named_buffers()}]
    moved = [(m._version > a, v._version > b) for (m, v), (a, b) in zip(stats, versions)]
    for _ in range(2):
        _clear(modg, Lg, Rg)
        _gpu_step(modg, *gpu)
    bufs.append({k: b.detach().cpu().clone() for k, b in modg.named_buffers()})
    masks = _masks_of(outs, modg)
    r64 = SB.stage0_grads_train(mod, *cpu, torch.float64, masks, steps=3)
    r32 = SB.stage0_grads_train(mod, *cpu, torch.float32, masks, steps=1)
    rows = {}
    for k, ref in r64["grads"].items():
        e_hip = float((got[k].double() - ref).abs().max())
        e_32 = float((r32["grads"][k].double() - ref).abs().max())
        gate = max(4.0 * e_32, 2e-5 * max(1.0, float(ref.abs().max())))
        rows[k] = {"hip_vs_f64": e_hip, "f32_vs_f64": e_32, "gate": gate, "ratio": e_hip / gate,
                   "max_abs_f64": float(ref.abs().max()), "shape_ok": got[k].shape == ref.shape}
    flips = [{"unit": i, "flips": n, "worst_abs_pre64": worst, "bound": bound}
             for i, (n, worst, bound) in enumerate(SG.flips_within_gate(r64, r32, TOL_WINO))]
    buffers = {}
    for steps, have in ((1, bufs[0]), (3, bufs[1])):
        want = r64["history"][steps - 1]
        assert want.keys() == have.keys()
        for k, ref in want.items():
            if k.endswith("num_batches_tracked"):
                buffers["%s after %d" % (k, steps)] = {"hip": int(have[k]), "f64": int(ref)}
            else:
                buffers["%s after %d" % (k, steps)] = {"ratio_to_FP32_TOL": MC.close(have[k], ref, MC.FP32_TOL)}
    # the eval forward after the steps: on the new statistics, and a fresh module loaded from the state_dict agrees bit for bit
    with torch.no_grad():
        pred_new = modg.eval().stage0(Lg, Rg, D)
        fresh = copy.deepcopy(mod).to(dev).eval()
        fresh.load_state_dict(modg.state_dict())
        pred_fresh = fresh.stage0(Lg, Rg, D)
    _PARITY[name] = {"tensors": rows, "flips": flips, "buffers": buffers, "calls": calls, "graph": names, "moved": moved,
                     "eval_forward": {"differs_from_old_statistics": not _bits_equal(pred_new, pred_old),
                                      "equals_fresh_module": _bits_equal(pred_new, pred_fresh)}}
    return _PARITY[name]


@pytest.mark.parametrize("name", sorted(SG.MODULE_CASES))
def test_module_against_float64(dev, name):
    """Every gradient (24 parameters + L + R) within the gate of the float64 train-mode run with the GPU's masks imposed; the
    imposed decisions within the forward gate of zero (`flips_within_gate`); running statistics and num_batches_tracked
    after 1 and 3 steps within MC.FP32_TOL of float64; the versions moved and the eval forward refolds.

    Measured on an MI355X (profiles/stage0_bn_train_parity.json), worst hip / gate per case: c8_cor 0.53
    (conv2.0.bn.weight), c12_ssd 0.99 (conv2.2.bn.weight: 1.98e-5 against the gate's floor 2e-5, float32 on the CPU 4.3e-6;
    the next tensor of the case 0.33), c216_cor 0.49 (conv0.0.bn.bias); no imposed decision differed from float64's; the
    buffers within 0.009 of FP32_TOL."""
    p = parity_ratios(name)
    calls, names = p["calls"], p["graph"]
    assert not [c for c in calls if "_stack_" in c or c.startswith("decnet_stage0_forward")], calls
    assert calls.count("decnet_conv3d_wgrad") == 8, calls
    assert calls.count("decnet_bn_train_cl_forward") == 8 and calls.count("decnet_bn_train_cl_backward") == 8, calls
    assert names.count("BatchNorm3dActFunctionBackward") == 8 and names.count("Conv3dFunctionBackward") == 8, names
    assert not _library_nodes(names), names
    assert len(p["tensors"]) == 2 + 8 * 3
    for k, row in p["tensors"].items():
        print(name, k, "hip %.3g  f32 %.3g  gate %.3g  ratio %.3g" % (row["hip_vs_f64"], row["f32_vs_f64"], row["gate"], row["ratio"]))
    for k, row in p["tensors"].items():
        assert row["shape_ok"] and row["hip_vs_f64"] <= row["gate"], (name, k, row)
    for row in p["flips"]:
        print(name, "unit %(unit)d: %(flips)d imposed decisions differ, worst |pre64| %(worst_abs_pre64).3g, gate %(bound).3g" % row)
        assert row["worst_abs_pre64"] <= row["bound"], (name, row)
    for k, row in p["buffers"].items():
        if "ratio_to_FP32_TOL" in row:
            assert row["ratio_to_FP32_TOL"] <= 1.0, (name, k, row)
        else:
            assert row["hip"] == row["f64"] == int(k.rsplit(" ", 1)[1]), (name, k, row)
    assert all(a and b for a, b in p["moved"]), p["moved"]
    assert p["eval_forward"]["differs_from_old_statistics"] and p["eval_forward"]["equals_fresh_module"], p["eval_forward"]


def test_frozen_units_inside_a_training_module(dev):
    """bn.eval() on two of the eight units of a module in .train() mode: those two run the frozen route (its bits, on the
    input the module gave them), their buffers and versions are untouched; the other six have moved."""
    from decnet_amd import Conv3dFunction, stage0, stage0_grad
    from decnet_amd.stage0 import fold_bn
    frozen = (1, 6)
    mod, modg, cpu, gpu = _on_gpu("c8_cor", dev, frozen)
    assert modg.training and not any(modg.units()[i].bn.training for i in frozen)
    before = [{k: (b.detach().clone(), b._version) for k, b in u.bn.named_buffers()} for u in modg.units()]
    pred, reg, outs, calls = _gpu_step(modg, *gpu)
    names = _graph_names(pred)
    assert names.count("BatchNorm3dActFunctionBackward") == 6 and names.count("Conv3dFunctionBackward") == 8, names
    assert calls.count("decnet_bn_train_cl_forward") == 6 and calls.count("decnet_conv3d_wgrad") == 8, calls
    variant = stage0.WINO_VARIANT.get(stage0.conv_algo(gpu[2]))
    for i, u in enumerate(modg.units()):
        for k, b in u.bn.named_buffers():
            same = torch.equal(b, before[i][k][0])
            if i in frozen:
                assert same and b._version == before[i][k][1], (i, k)
            else:
                assert not same, (i, k)
                assert k == "num_batches_tracked" or b._version > before[i][k][1], (i, k)
        if i in frozen:
            with torch.no_grad():
                scale, shift = fold_bn(u.bn)
                want = Conv3dFunction.apply(stage0_grad.unit_operands(u.conv.weight.detach(), variant), bool(u.relu),
                                            u.conv.weight, scale, shift, outs[i - 1])
            assert _bits_equal(outs[i], want), "unit %d is not on the frozen route" % i
    assert all(p.grad is not None for p in modg.parameters())
    masks = _masks_of(outs, modg)
    r64 = SB.stage0_grads_train(mod, *cpu, torch.float64, masks, frozen=frozen)
    r32 = SB.stage0_grads_train(mod, *cpu, torch.float32, masks, frozen=frozen)
    for k, t in _leaves(modg, gpu[0], gpu[1]).items():
        ref = r64["grads"][k]
        gate = max(4.0 * float((r32["grads"][k].double() - ref).abs().max()), 2e-5 * max(1.0, float(ref.abs().max())))
        assert float((t.grad.cpu().double() - ref).abs().max()) <= gate, k


def test_graphed_train_step(dev):
    """A train-mode step captured once as a GraphedStep and replayed on three batches copied in place: every replay's
    gradients have the bits of an eager step on that batch, and -- the buffers put back to the start past the warm-up --
    three replays leave the buffers of three eager steps, bit for bit."""
    import decnet_amd
    from decnet_amd.graphs import GraphedStep
    gen = torch.Generator().manual_seed(5)

    def setup():
        _, modg, _, (Lg, Rg, D, r, r2) = _on_gpu("c8_cor", dev)
        leaves = list(_leaves(modg, Lg, Rg).values())

        def step():
            with decnet_amd.hip_grad():
                pred, reg = modg.stage0(Lg, Rg, D, return_reg=True)
            ((pred * r).sum() + (reg * r2).sum()).backward()
        return modg, Lg, Rg, leaves, step

    me, Le, Re, le, step_e = setup()
    data = [(Le.detach().cpu(), Re.detach().cpu())]             # the captured batch first, then two new ones
    data += [tuple(torch.relu(torch.randn(Le.shape, generator=gen)) for _ in range(2)) for _ in range(2)]
    eager = []
    for a, b in data:
        with torch.no_grad():
            Le.copy_(a)
            Re.copy_(b)
        for p in le:
            p.grad = None
        step_e()
        torch.cuda.synchronize()
        eager.append([p.grad.detach().clone() for p in le])
    assert not all(_bits_equal(x, y) for x, y in zip(eager[0], eager[1])), "the new data changed nothing"
    mg, Lg, Rg, lg, step_g = setup()
    start = {k: b.detach().clone() for k, b in mg.named_buffers()}
    graphed = GraphedStep(step_g, grads_of=lg)
    with torch.no_grad():                                       # the warm-up steps moved the buffers: back to the start
        for k, b in mg.named_buffers():
            b.copy_(start[k])
    for (a, b), want in zip(data, eager):
        with torch.no_grad():
            Lg.copy_(a)
            Rg.copy_(b)
        for p in lg:
            p.grad.fill_(float("nan"))
        graphed()
        torch.cuda.synchronize()
        for p, w in zip(lg, want):
            assert _bits_equal(p.grad, w), "a replay's gradient differs from the eager step's"
    be = dict(me.named_buffers())
    for k, b in mg.named_buffers():
        assert torch.equal(b, be[k]) and not torch.equal(b, start[k]), k
        if k.endswith("num_batches_tracked"):
            assert int(b) == 3


def test_refusals_on_the_gpu(dev):
    import decnet_amd
    _, modg, _, (Lg, Rg, D, r, r2) = _on_gpu("c8_cor", dev)
    before = {k: b.detach().clone() for k, b in modg.named_buffers()}
    with pytest.raises(NotImplementedError, match="hip_grad"):                  # hip_grad() off
        modg.stage0(Lg, Rg, D)
    with decnet_amd.hip_grad(), torch.no_grad(), pytest.raises(NotImplementedError, match="hip_grad"):
        modg.stage0(Lg, Rg, D)
    with decnet_amd.hip_grad(), pytest.raises(NotImplementedError):             # a CPU input
        modg.stage0(Lg.detach().cpu().requires_grad_(), Rg, D)
    m = copy.deepcopy(modg)
    m.units()[5].bn.momentum = None                                            # a cumulative average
    with decnet_amd.hip_grad(), pytest.raises(NotImplementedError, match="momentum"):
        m.stage0(Lg, Rg, D)
    for k, b in m.named_buffers():                                              # refused before unit 0 wrote a statistic
        assert torch.equal(b, before[k]), k
    m = copy.deepcopy(modg)
    m.units()[2].bn = torch.nn.BatchNorm3d(8, track_running_stats=False).to(dev)
    with decnet_amd.hip_grad(), pytest.raises(NotImplementedError, match="track_running_stats"):
        m.stage0(Lg, Rg, D)
    m = copy.deepcopy(modg)
    m.units()[2].bn = torch.nn.BatchNorm3d(8, affine=False).to(dev)
    with decnet_amd.hip_grad(), pytest.raises(NotImplementedError, match="affine"):
        m.stage0(Lg, Rg, D)
    cat = decnet_amd.CostRegNetNoDown(8, 16, "cat").to(dev).train()
    with decnet_amd.hip_grad(), pytest.raises(NotImplementedError, match="cat"):
        cat.stage0(Lg, Rg, D)
    for k, b in modg.named_buffers():
        assert torch.equal(b, before[k]), k
    with decnet_amd.hip_grad():                                                 # and the very same module, asked properly, runs
        assert modg.stage0(Lg, Rg, D).grad_fn is not None
