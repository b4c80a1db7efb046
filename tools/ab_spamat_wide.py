#!/usr/bin/env python
"""A/B timing of the wide-disparity SpaMat / SpaVar path (csrc/spamat_wide.hip): the caller-workspace (`_ws`) entries
against the legacy entries of a PARENT build of the library, eagerly and as HIP-graph replays.

    python tools/ab_spamat_wide.py --parent-lib /path/to/parent/libdecnet_hip.so [--out profiles/ab_spamat_wide.json]

Planes: stage 3 of tests/golden/inputdata/real/00003 (max_disp 405) and real/00004 (621) as decnet_amd.demo.run_pair
pads them (1 x 8 x 729 x 1296), features and detail masks from the demo's seeded from-scratch network; made once by a
child process (`--prepare`) and stored beside the results.  That network's masks are sparse (about 2 % of the pixels);
`--density P` replaces them by Bernoulli(P) masks on the same features (dense rows take other band kernels).

Work: the fused SpaMat + SpaVar forward and the SpaMat backward.  Legs, each a fresh child process (DECNET_HIP_LIB is read
once per process), parent and new alternating, `--repeats` rounds:
    legacy_eager     bit-mask forward entry / backward entry, one call after the other on the stream
    ws_eager         their `_ws` twins on a workspace allocated once                                   (new library only)
    legacy_captured  the calls captured into a HIP graph; the legacy entries decline there, so this is the float-mask
                     forward and the backward on the row-tile kernels: what a captured model falls back to
    ws_captured      the `_ws` calls captured into a HIP graph (bit-mask entry for the forward)         (new library only)
Time is device events around `--calls` calls (eager) or graph replays of one call each, after a warm-up.  Every leg also
dumps its outputs; the report says whether the new library's legs equal the parent's legacy eager leg bit for bit."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PLANES = {"real/00003": 405, "real/00004": 621}
LEGS = ("legacy_eager", "ws_eager", "legacy_captured", "ws_captured")


def unpack_bits(bits, W):
    import torch
    B, H, wpr = bits.shape
    sh = torch.arange(64, device=bits.device, dtype=torch.int64)
    return ((bits.unsqueeze(-1) >> sh) & 1).reshape(B, H, wpr * 64)[:, :, :W].float().contiguous()


def pack_bits(m):
    """float 0/1 [B,H,W] -> int64 [B,H,ceil(W/64)], bit i of word w = pixel 64 w + i, zeros past W"""
    import torch
    B, H, W = m.shape
    wpr = (W + 63) // 64
    on = torch.zeros(B, H, wpr * 64, dtype=torch.int64, device=m.device)
    on[..., :W] = (m != 0).long()
    sh = torch.arange(64, device=m.device, dtype=torch.int64)
    return (on.view(B, H, wpr, 64) << sh).sum(-1).contiguous()          # (bit 63 wraps into the sign: the same 64 bits)


def prepare(work, density=None):
    """The stage-3 inputs of both planes -> work/plane_<D>.pt"""
    import torch
    from decnet_amd import demo
    import decnet_amd.model as M
    dev = torch.device("cuda:0")
    args = demo.build_parser().parse_args(["--cost_func", "cor"])
    torch.manual_seed(args.seed)
    model = demo.build_model(args, dev)
    orig = M.spamatvar_forward_bits
    for name, D in PLANES.items():
        d = os.path.join(ROOT, "tests", "golden", "inputdata", name)
        assert demo.read_ndisp(os.path.join(d, "calib.txt")) == D
        grabbed = {}

        def grab(L, R, lb, rb, Dc, out=None):
            if int(Dc) == D:
                grabbed.update(L=L.clone(), R=R.clone(), lbits=lb.clone(), rbits=rb.clone())
            return orig(L, R, lb, rb, Dc, out=out)
        M.spamatvar_forward_bits = grab
        try:
            demo.run_pair(model, demo.read_rgb(os.path.join(d, "im0.png")), demo.read_rgb(os.path.join(d, "im1.png")), dev, D)
        finally:
            M.spamatvar_forward_bits = orig
        torch.cuda.synchronize()
        W = grabbed["L"].shape[-1]
        grabbed["lmask"], grabbed["rmask"] = unpack_bits(grabbed["lbits"], W), unpack_bits(grabbed["rbits"], W)
        g = torch.Generator().manual_seed(D)
        if density is not None:
            for side in "lr":
                mk = (torch.rand(grabbed[side + "mask"].shape, generator=g) < density).float().to(dev)
                grabbed[side + "mask"], grabbed[side + "bits"] = mk, pack_bits(mk)
                assert torch.equal(unpack_bits(grabbed[side + "bits"], W), mk)
        grabbed["gout"] = torch.randn(grabbed["lmask"].shape, generator=g).to(dev)
        torch.save({k: v.cpu() for k, v in grabbed.items()}, os.path.join(work, "plane_%d.pt" % D))
        print("plane %s: features %s, max_disp %d, mask density %.3f / %.3f" % (
            name, tuple(grabbed["L"].shape), D, float(grabbed["lmask"].mean()), float(grabbed["rmask"].mean())), flush=True)


def run_leg(leg, work, tag, calls, warmup):
    """One leg on both planes with the library this process loaded -> JSON line; outputs -> work/out_<tag>_<D>.pt"""
    import ctypes
    import torch
    from decnet_amd import _lib
    # the library DECNET_HIP_LIB names (the parent's has no `_ws` symbols, so only what this leg calls is bound)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    ws_leg, captured = leg.startswith("ws_"), leg.endswith("_captured")
    used = ["decnet_spamatvar_forward_bits", "decnet_spamatvar_forward", "decnet_spamat_backward"]
    if ws_leg:
        used += ["decnet_spamat_workspace_floats", "decnet_spamatvar_forward_bits_ws", "decnet_spamat_backward_ws"]
    for name in used:
        fn = getattr(lib, name)
        fn.argtypes = _lib.SIGNATURES[name]
        fn.restype = ctypes.c_size_t if name.endswith("_floats") else ctypes.c_int
    dev = torch.device("cuda:0")
    res = {"leg": leg, "planes": {}}
    for D in PLANES.values():
        x = {k: v.to(dev) for k, v in torch.load(os.path.join(work, "plane_%d.pt" % D)).items()}
        B, C, H, W = x["L"].shape
        dims = (B, C, H, W, D)
        st = lambda: torch.cuda.current_stream().cuda_stream    # noqa: E731  (the capture runs on a stream of its own)
        pl = lambda: torch.full((B, H, W), float("nan"), device=dev)          # noqa: E731
        o, v, s, m = pl(), pl(), pl(), pl()
        gl, gr = torch.full_like(x["L"], float("nan")), torch.full_like(x["R"], float("nan"))
        p = lambda t: t.data_ptr()                                             # noqa: E731
        # the forward's outputs feed the backward: made once, by the library's eager legacy forward
        rc = lib.decnet_spamatvar_forward_bits(p(x["L"]), p(x["R"]), p(x["lbits"]), p(x["rbits"]), p(o), p(v), p(s), p(m),
                                               *dims, st())
        assert rc == 0, rc
        torch.cuda.synchronize()
        fo, fs, fm = o.clone(), s.clone(), m.clone()
        wsf = wsb = None
        if ws_leg:
            nf, nb = (int(lib.decnet_spamat_workspace_floats(*dims, w)) for w in (3, 4))
            wsf, wsb = torch.empty(nf, device=dev), torch.empty(nb, device=dev)

        def forward():
            if ws_leg:
                return lib.decnet_spamatvar_forward_bits_ws(p(x["L"]), p(x["R"]), p(x["lbits"]), p(x["rbits"]), p(o), p(v),
                                                            p(s), p(m), *dims, p(wsf), wsf.numel(), st())
            if captured:                                   # the legacy bit-mask entry declines: the model's fallback
                return lib.decnet_spamatvar_forward(p(x["L"]), p(x["R"]), p(x["lmask"]), p(x["rmask"]), p(o), p(v), p(s),
                                                    p(m), *dims, st())
            return lib.decnet_spamatvar_forward_bits(p(x["L"]), p(x["R"]), p(x["lbits"]), p(x["rbits"]), p(o), p(v), p(s),
                                                     p(m), *dims, st())

        def backward():
            a = (p(x["L"]), p(x["R"]), p(x["lmask"]), p(x["rmask"]), p(fo), p(fs), p(fm), p(x["gout"]), p(gl), p(gr))
            if ws_leg:
                return lib.decnet_spamat_backward_ws(*a, *dims, p(wsb), wsb.numel(), st())
            return lib.decnet_spamat_backward(*a, *dims, st())

        times = {}
        for name, fn in (("fused_forward", forward), ("spamat_backward", backward)):
            assert fn() == 0                               # eager once: loads the code objects
            torch.cuda.synchronize()
            if captured:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    rc = fn()
                assert rc == 0, rc
                go = graph.replay
            else:
                go = fn
            for _ in range(warmup):
                go()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                go()
            e1.record()
            torch.cuda.synchronize()
            times[name] = e0.elapsed_time(e1) / calls
        res["planes"][str(D)] = times
        torch.save({k: t.cpu() for k, t in (("out", o), ("var", v), ("S", s), ("max", m), ("gl", gl), ("gr", gr))},
                   os.path.join(work, "out_%s_%d.pt" % (tag, D)))
    print("LEG " + json.dumps(res), flush=True)


def child(argv, env=None, timeout=600):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, env=dict(os.environ, **(env or {})),
                       capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit("child %s failed (%d):\n%s\n%s" % (argv, r.returncode, r.stdout[-2000:], r.stderr[-3000:]))
    return r.stdout


def same_bits(a, b):
    import torch
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdecnet_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_spamat_wide.json"))
    ap.add_argument("--work", default=None, help="directory for the plane inputs and the legs' outputs")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--density", type=float, default=None, help="Bernoulli masks of this density instead of the network's")
    ap.add_argument("--prepare", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--leg", choices=LEGS, help=argparse.SUPPRESS)
    ap.add_argument("--tag", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.prepare:
        return prepare(a.work, a.density)
    if a.leg:
        return run_leg(a.leg, a.work, a.tag, a.calls, a.warmup)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: a build of the parent commit's library is the yardstick")
    import torch
    work = a.work or tempfile.mkdtemp(prefix="ab_spamat_wide_")
    os.makedirs(work, exist_ok=True)
    dens = ["--density", str(a.density)] if a.density is not None else []
    print(child(["--prepare", "--work", work] + dens, timeout=900), end="", flush=True)
    runs = []
    order = [("parent", "legacy_eager"), ("new", "legacy_eager"), ("new", "ws_eager"), ("parent", "legacy_captured"),
             ("new", "legacy_captured"), ("new", "ws_captured")]
    for rep in range(a.repeats):
        for which, leg in order:
            tag = "%s_%s" % (which, leg)
            env = {"DECNET_HIP_LIB": os.path.abspath(a.parent_lib)} if which == "parent" else {}
            out = child(["--leg", leg, "--tag", tag, "--work", work, "--calls", str(a.calls), "--warmup", str(a.warmup)], env)
            line = [ln for ln in out.splitlines() if ln.startswith("LEG ")][-1]
            r = json.loads(line[4:])
            r.update(library=which, repeat=rep)
            runs.append(r)
            print("%d %-7s %-16s %s" % (rep, which, leg, json.dumps(r["planes"])), flush=True)
    # medians, ratios, bit-identity
    report = {"calls": a.calls, "warmup": a.warmup, "repeats": a.repeats, "unit": "ms per call", "runs": runs, "planes": {},
              "masks": "the seeded network's" if a.density is None else "Bernoulli(%g)" % a.density}
    for D in map(str, PLANES.values()):
        tab = {}
        for which, leg in order:
            for op in ("fused_forward", "spamat_backward"):
                v = sorted(r["planes"][D][op] for r in runs if r["library"] == which and r["leg"] == leg)
                tab.setdefault(op, {})["%s_%s" % (which, leg)] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}
        ref = torch.load(os.path.join(work, "out_parent_legacy_eager_%s.pt" % D))
        bits = {"%s_%s" % (w, leg): same_bits(ref, torch.load(os.path.join(work, "out_%s_%s_%s.pt" % (w, leg, D))))
                for w, leg in order}
        req = {}
        for op, t in tab.items():
            pe, pc = t["parent_legacy_eager"]["median"], t["parent_legacy_captured"]["median"]
            we, wc = t["new_ws_eager"]["median"], t["new_ws_captured"]["median"]
            req[op] = {"ws_eager_over_parent_eager": we / pe, "ws_eager_ok": we <= 1.05 * pe,
                       "ws_captured_over_parent_eager": wc / pe, "ws_captured_ok": wc <= 1.10 * pe and wc < pc,
                       "parent_captured_over_ws_captured": pc / wc}
        report["planes"][D] = {"ms": tab, "equals_parent_legacy_eager_bit_for_bit": bits, "requirements": req}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({D: report["planes"][D]["requirements"] for D in report["planes"]}, indent=1))
    print("bit-identity:", json.dumps({D: report["planes"][D]["equals_parent_legacy_eager_bit_for_bit"]
                                       for D in report["planes"]}))


if __name__ == "__main__":
    main()
