"""Timing of the refine model (hierdiff_amd.refine.Node2Vec, H = 256, n_layers 2, vocab 780): check_node over every node of a
tree of 10 / 20 / 30 nodes (what check_tree does per call), one training step at batch 32 (forward, backward, AdamW), and the same
two workloads as eager torch ops on the same GPU (tests/refine_oracle.py with the oracle's tensors kept on the device).

    python scratch/refine_timing.py [out.json]        # default profiles/refine_timing.json
"""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from hierdiff_amd.refine import Node2Vec, get_bfs_depth_edges, synthetic_refine_state_dict  # noqa: E402
from oracle import egnn_oracle as orc  # noqa: E402
from tests import refine_oracle as ro  # noqa: E402

DEV = "cuda:0"
H, L = 256, 2


def timed(fn, warm=2, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "reps": reps}


def random_adj(rng, n):
    adj = np.zeros((n, n), np.int64)
    for i in range(1, n):
        p = int(rng.integers(0, i))
        adj[i, p] = adj[p, i] = 1
    return adj


def tree(rng, n, vocab):
    keys = sorted({s for s in vocab.mol_sizes if 0 < s < 26 and len(vocab.get_size(s)) >= 2})
    nodes = []
    for _ in range(n):
        s = int(rng.choice(keys))
        nodes.append(ro.MolTreeNode(int(rng.choice(vocab.get_size(s))), s, 2 * rng.standard_normal(3), rng.standard_normal(10)))
    return nodes, torch.tensor(random_adj(rng, n)).nonzero().T.tolist()


def batch(rng, size_dict, n_list):
    keys = sorted(k for k in size_dict if k < 26)
    bs, nmax = len(n_list), max(n_list)
    b = {k: np.zeros(s, t) for k, s, t in (("feature", (bs, nmax, 8), np.float32), ("vocab", (bs, nmax), np.int64),
                                            ("size", (bs, nmax), np.int64), ("pos", (bs, nmax, 3), np.float32),
                                            ("mask", (bs, nmax, 1), np.float32), ("label", (bs,), np.int64), ("val", (bs,), np.float32))}
    per, pred = [], []
    for i, n in enumerate(n_list):
        adj = random_adj(rng, n)
        p = int(rng.integers(0, n))
        sizes = [int(rng.choice(keys)) for _ in range(n)]
        wids = [int(rng.choice(size_dict[s])) for s in sizes]
        b["size"][i, :n], b["vocab"][i, :n], b["mask"][i, :n] = sizes, wids, 1
        b["feature"][i, :n] = rng.standard_normal((n, 8))
        b["pos"][i, :n] = 2 * rng.standard_normal((n, 3))
        b["label"][i], b["vocab"][i, p], b["feature"][i, p], b["val"][i] = wids[p], 780, 0, adj.sum(1)[p]
        per.append(get_bfs_depth_edges(torch.tensor(adj).nonzero().T.tolist(), p, n))
        pred.append(p)
    edges = [[[], []] for _ in range(max(len(e) for e in per))]
    for i, e in enumerate(per):
        for j, (a, c) in enumerate(e):
            edges[j][0].extend(x + i * nmax for x in a)
            edges[j][1].extend(x + i * nmax for x in c)
    out = {k: torch.from_numpy(v) for k, v in b.items()}
    out.update(edges=edges, predict_idx=pred)
    return out


def main(path):
    size_dict, mol_sizes = ro.load_size_dict()
    vocab = ro.StubVocab(mol_sizes)
    sd_np = synthetic_refine_state_dict(780, 8, H, L, 0)
    m = Node2Vec(size_dict, 780, 8, H, L)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()})
    m = m.to(DEV)
    sd = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in sd_np.items()}
    orc._t = lambda a: a if isinstance(a, torch.Tensor) and a.is_floating_point() else torch.as_tensor(a, dtype=torch.float32)
    rng = np.random.Generator(np.random.PCG64(1))
    out = {"config": {"hidden_size": H, "n_layers": L, "vocab_size": 780, "device": torch.cuda.get_device_name(0)},
           "check_node": {}, "train_step_b32": {}}
    for n in (10, 20, 30):
        nodes, edges = tree(rng, n, vocab)
        idx, wid = list(range(n)), [nd.wid for nd in nodes]
        hip = timed(lambda: m.check_node(vocab, nodes, edges, idx, wid, DEV))
        with torch.no_grad():
            eager = timed(lambda: ro.check_node(sd, L, vocab, nodes, edges, idx, wid), reps=5)
            a = np.asarray([float(r[0]) for r in m.check_node(vocab, nodes, edges, idx, wid, DEV)])
            b = ro.check_node(sd, L, vocab, nodes, edges, idx, wid)[0]
        out["check_node"][f"n{n}"] = {"hip": hip, "eager_torch": eager, "copies": n,
                                      "logp_rel_l2_vs_eager": float(np.linalg.norm(a - b) / np.linalg.norm(b))}
        print(n, out["check_node"][f"n{n}"], flush=True)
    bt = batch(rng, size_dict, [int(rng.integers(8, 21)) for _ in range(32)])
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=4e-4, weight_decay=1e-8, amsgrad=True)

    def hip_step():
        opt.zero_grad(set_to_none=True)
        m(bt)["loss"].backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
    out["train_step_b32"]["hip"] = timed(hip_step, reps=5)
    sdp = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    opt2 = torch.optim.AdamW(list(sdp.values()), lr=4e-4, weight_decay=1e-8, amsgrad=True)
    dev_bt = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in bt.items()}

    def eager_step():
        opt2.zero_grad(set_to_none=True)
        ro.forward(sdp, size_dict, L, dev_bt)["loss"].backward()
        torch.nn.utils.clip_grad_norm_(list(sdp.values()), 1.0)
        opt2.step()
    out["train_step_b32"]["eager_torch"] = timed(eager_step, reps=5)
    out["train_step_b32"]["nodes"] = int(bt["mask"].sum())
    print(out["train_step_b32"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "refine_timing.json"))
