#!/usr/bin/env python
"""The gradient parity of one training stage end to end (tests/test_stage_step_gpu.py, test c) as numbers: per case and
tensor max|g_hip - g64|, max|g32 - g64|, the gate max(4 max|g32 - g64|, 2e-5 max(1, max|g64|)) (L and R: + 5e-5 max|g_sp|),
their ratio and the error as a share of max|g64|; the ReLU decisions and warp cells the reference took from the GPU run.

    python tools/stage_step_parity.py [--out profiles/stage_step_parity.json]

No timing.  Needs the GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage_step_parity.json"))
    a = ap.parse_args()
    import torch
    import decnet_amd
    if not torch.cuda.is_available():
        raise SystemExit("stage_step_parity.py measures on the GPU; there is none")
    import test_stage_step_gpu as T
    cases = {name: T.parity_ratios(name) for name in sorted(T.S.CASES)}
    worst = {name: max(c["tensors"].items(), key=lambda kv: kv[1]["ratio"]) for name, c in cases.items()}
    rep = {"what": "max|g_hip - g64|, max|g32 - g64|, the gate max(4 max|g32 - g64|, 2e-5 max(1, max|g64|)) (+ 5e-5 max|g_sp| "
                   "for L and R), ratio = hip_vs_f64 / gate, rel = hip_vs_f64 / max|g64|, per tensor of one training stage",
           "device": torch.cuda.get_device_name(0), "version": decnet_amd.version(),
           "worst_hip_over_gate": {n: {"tensor": k, "ratio": r["ratio"]} for n, (k, r) in worst.items()},
           "worst_rel": {n: max(r["rel"] for r in c["tensors"].values()) for n, c in cases.items()}, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: rep[k] for k in ("worst_hip_over_gate", "worst_rel")}))


if __name__ == "__main__":
    main()
