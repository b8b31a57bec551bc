#!/usr/bin/env python3
"""Generate tests/golden/complete_encode.npz: the reference's own `attribute_converter(in_encoding='int', out_encoding=...)`
(R/utils/attribute_code.py:13, :240-304) on small integer graphs -- the pin of `dsg_encode` / `diffusesg_amd.io.encode`.

DEV-CONTAINER ONLY, like tools/gen_golden.py: the reference tree does not exist where the tests run; only the arrays written here
are committed.  The reference is imported with the same three-symbol `timm` stand-in (its utils package does not need more).

Per encoding `enc` in bits / one_hot / ddpm the file holds, for B = 3 graphs of N = 8 nodes with 8 / 5 / 1 valid ones:
  {enc}_q_adj [B,N,N] int32, {enc}_q_node [B,N] int32   integer types (0 at padded nodes and on the diagonal), every type occurs
  {enc}_adj, {enc}_node float32                         the reference's outputs, called the way its data loader calls it
                                                        (R/utils/dataloader.py:189-200: float32 integer tensors in, DDPM range out)
  {enc}_types int32 [2]                                 (n_adj_type, n_node_type)
and flags [B,N] bool.

Usage:  python tools/gen_complete_golden.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from diffusesg_amd import weights as W       # noqa: E402

N, B, VALID = 8, 3, [8, 5, 1]
# (n_adj_type, n_node_type): Visual Genome's counts for 'bits' (6 / 8 digits); small ones for the per-type-channel encodings
TYPES = {"bits": (51, 150), "one_hot": (7, 11), "ddpm": (7, 11)}


def int_case(enc: str):
    """flags, q_adj, q_node of one encoding: hashed integers with every type present, masked like the data loader pads them."""
    n_adj_type, n_node_type = TYPES[enc]
    flags = W.synth_flags(B, N, VALID)
    q_adj = (W.uniform01(5, f"cenc/{enc}/adj", B * N * N) * n_adj_type).astype(np.int32).reshape(B, N, N)
    q_node = (W.uniform01(5, f"cenc/{enc}/node", B * N) * n_node_type).astype(np.int32).reshape(B, N)
    q_adj[0].reshape(-1)[1:1 + n_adj_type] = np.arange(n_adj_type)          # sample 0 is full: every edge type, 0 and the last one
    q_node[0, :2] = (0, n_node_type - 1)
    q_adj[:, np.arange(N), np.arange(N)] = 0
    f = flags.astype(np.int32)
    return flags, q_adj * f[:, :, None] * f[:, None, :], q_node * f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    import gen_golden
    gen_golden._import_reference()
    from utils.attribute_code import attribute_converter
    res = {}
    for enc, (n_adj_type, n_node_type) in TYPES.items():
        flags, q_adj, q_node = int_case(enc)
        fl = torch.from_numpy(flags)
        adj = attribute_converter(torch.tensor(q_adj, dtype=torch.float32), fl, in_encoding="int", out_encoding=enc,
                                  num_attr_type=n_adj_type, flag_adjs=True, flag_in_ddpm_range=False, flag_out_ddpm_range=True)
        node = attribute_converter(torch.tensor(q_node, dtype=torch.float32), fl, in_encoding="int", out_encoding=enc,
                                   num_attr_type=n_node_type, flag_nodes=True, flag_in_ddpm_range=False, flag_out_ddpm_range=True)
        assert adj.dtype == torch.float32 and node.dtype == torch.float32, (adj.dtype, node.dtype)
        res["flags"] = flags
        res[f"{enc}_q_adj"], res[f"{enc}_q_node"] = q_adj, q_node
        res[f"{enc}_adj"], res[f"{enc}_node"] = adj.numpy(), node.numpy()
        res[f"{enc}_types"] = np.array([n_adj_type, n_node_type], np.int32)
        print(enc, tuple(adj.shape), tuple(node.shape))
    path = os.path.join(args.out, "complete_encode.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
