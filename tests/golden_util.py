"""Helpers to read the committed golden fixtures (data only: inputs + expected outputs)."""
import glob
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden_npz(stem):
    """The arrays of tests/golden/<stem>.npz, or of <stem>.part<i>.npz when the fixture is stored in parts (a committed file stays
    under 1 MiB): an array too large for one part is stored as row blocks "<key>#<j>" and joined again along axis 0."""
    whole = os.path.join(GOLDEN, f"{stem}.npz")
    paths = [whole] if os.path.exists(whole) else sorted(glob.glob(os.path.join(GOLDEN, f"{stem}.part*.npz")))
    if not paths:
        raise FileNotFoundError(whole)
    arrays = {}
    for p in paths:
        with np.load(p) as z:
            arrays.update({k: z[k] for k in z.files})
    blocks = {}
    for k in [k for k in arrays if "#" in k]:
        base, j = k.rsplit("#", 1)
        blocks.setdefault(base, []).append((int(j), arrays.pop(k)))
    for base, parts in blocks.items():
        arrays[base] = np.concatenate([a for _, a in sorted(parts, key=lambda t: t[0])], axis=0)
    return arrays


def load_net_golden(name):
    z = load_golden_npz(f"net_{name}")
    cfg = json.loads(str(z["cfg_json"]))
    sd = {}
    for k in z:
        if k.startswith("sd::"):
            sd[k[4:]] = torch.from_numpy(z[k])
        elif k.startswith("sdseed::"):
            seed, scale = z[k]
            g = torch.Generator().manual_seed(int(seed))
            sd[k[8:]] = (float(scale) * torch.randn(4672, 4096, generator=g)).half().float()
    ssl = {k[4:]: z[k] for k in z if k.startswith("ssl_")}
    return cfg, sd, z["x"], z["p"], z["v"], ssl


NET_CASES = ["gn_silu_preact", "gn_dense_leaky", "bn_relu_postact", "stride2"]

SEEDED_NET_CASES = ["r320x7_seeded"]


def load_seeded_net_golden(name):
    """Full-width fixtures (tools/gen_golden_net.py::SEEDED_CASES): cfg, seed, x and the outputs of the REFERENCE module with the
    weights `matrix0_amd.weights.random_state_dict(cfg, seed, varied=True)` loaded into it; the weights are rebuilt here."""
    from matrix0_amd.weights import random_state_dict
    z = np.load(os.path.join(GOLDEN, f"net_{name}.npz"))
    cfg = json.loads(str(z["cfg_json"]))
    sd = random_state_dict(cfg, seed=int(z["seed"]), varied=True)
    ssl = {k[4:]: z[k] for k in z.files if k.startswith("ssl_")}
    return cfg, sd, z["x"], z["p"], z["v"], ssl
