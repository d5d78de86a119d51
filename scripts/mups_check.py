"""How far the MuPS kernels (csrc/mups.hip) are from the float64 restatement on the crafted cases of tests/_mups_fixture.py, in units of
the bound the tests hold them to (4 e32 + 2^-22, e32 = the float32 restatements' own error).  Per grid and case: the largest e32, the
share of ill-conditioned cells (bound > 5e-6), the largest error / bound of the dense f32 run over all outputs and over the
well-conditioned cells, and where the latter sits (row, n_eff, scale, statistic, Gaussian).  The tests gate the same numbers
(tests/test_gpu_mups_cases.py); this records them.  Writes one JSON object (default: profiles/mups_check.json).

    python scripts/mups_check.py [--out profiles/mups_check.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import nesti_net_amd  # noqa: E402,F401
import _mups_fixture as F  # noqa: E402
from nesti_net_amd.model import mups_forward  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mups_check.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for grid in F.GRIDS:
        for kind in F.KINDS + ("layout",):
            c = F.layout_case(grid) if kind == "layout" else F.case(grid, kind)
            got = mups_forward(F.config(grid, c["S"], c["P"]), torch.as_tensor(c["pts"], device=dev), torch.as_tensor(c["n_eff"], device=dev))
            r = F.ratios(got.cpu().numpy(), c)
            well = np.where(c["ill"][:, None, None, None, :, :], 0.0, r)
            b, i, j, k, s, ch = (int(x) for x in np.unravel_index(np.argmax(well), well.shape))
            rows.append({"grid": grid, "case": kind, "S": c["S"], "P": c["P"], "largest_e32": float(c["e32"].max()),
                         "median_bound": float(np.median(c["bound"])), "largest_bound": float(c["bound"].max()),
                         "ill_conditioned_share": float(c["ill"].mean()), "largest_error_over_bound": float(r.max()),
                         "largest_error_over_bound_well_conditioned": float(well.max()),
                         "at": {"row": b, "n_eff": int(c["n_eff"][b, s]), "scale": s, "statistic": F.STATS[ch], "gaussian": [i, j, k]}})
            print(rows[-1])
    out = {"device": torch.cuda.get_device_name(dev), "bound": "4 e32 + 2^-22", "ill_conditioned_above": F.ILL, "seed": F.SEED, "cases": rows,
           "largest_error_over_bound": max(r["largest_error_over_bound"] for r in rows)}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
