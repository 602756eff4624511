"""Refine model `Node2Vec` on MI355X - drop-in for models/model_refine.py of the reference (HierDiff's decoder: `check_tree`
re-scores every fragment of a finished tree and swaps out one it finds unlikely; generation/ar_sampling.py:38,331-362).

Same constructor (`size_dict` a pickle path as in the reference, or a dict), same `state_dict` keys / shapes / order, same
`forward(batch)` on data_utils/dataset_refine.py:PadCollate's dict, `check_node`, `check_tree`, `check_final_tree`, and the module
helpers `get_bfs_depth_edges` / `flat_add_and_concat`.  Arithmetic (exact fp32, no CPU fallback):
  * input stage: `hd_refine_embed_forward` gathers v_embedding / size_embedding rows into column blocks 0 and 2 of the [M][3H]
    projection input, the f_embedding MLP writes block 1 in place (hd_gemm_f32 with a row stride of 3H), projection on hd_gemm_f32;
  * message passing: the stage-2 layer `stage2.E_GCL`; the edge attribute |x_row - x_col|^2 before every layer call is
    `hd_sqdist_forward` / `_backward` on the layer's own edge graph;
  * head: Linear + SiLU + Linear on hd_gemm_f32, then the size-restricted softmax `hd_cand_xent_forward` / `_backward` (loss,
    accuracy, check_node's log-probabilities and top-k candidates).
When autograd is recording and a parameter requires grad, `forward` is differentiable end to end (autograd Functions over those
kernels, training._Linear, stage2._EgclFunction); otherwise every call takes the inference path.

The RDKit / JT-VAE steps of check_tree / check_final_tree go through `set_chem_hooks` (the defaults import rdkit and
generation.jtnn.jtnn_dec lazily, only when an edit needs them).  Nodes count as "exact" when their class is named MolTreeNode.
Reference quirks kept: check_num shrinks for every later row once one row has fewer candidates; a label / pad_wid outside its
candidate set raises ValueError; a size >= 26 raises IndexError before any launch; a size without candidates raises TypeError (the
reference's handle_wrong_sizes call lacks an argument); an empty depth list leaves h and x unchanged.  An empty per-depth edge list
([[], []]), which the reference cannot run either, raises ValueError.
"""
from __future__ import annotations

import copy
import hashlib
import math
import os
import pickle
from collections import OrderedDict, deque
from typing import Dict, List, Sequence

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import HierDiffHipError
from .stage2 import E_GCL, egcl_param_shapes, synthetic_egcl_state_dict
from .training import _EPI_BIAS_SILU2, _EPI_MUL_DSILU, _Linear, _gemm, _linear_dw, _linear_dx, _linear_fwd

MASK_TOKEN = 780        # the "masked node" id check_node writes at the scored position (model_refine.py hard-codes it)
N_SIZES = 26            # rows of size_embedding
MAX_TOPK = 16           # candidates hd_cand_xent_forward returns per row
_KINDS = ("collect", "reverse", "back")


# ----------------------------------------------------------------------------- chemistry hooks of check_tree / check_final_tree
_HOOKS: Dict[str, object] = {"mol_from_smiles": None, "can_assemble": None}


def set_chem_hooks(mol_from_smiles=None, can_assemble=None) -> Dict[str, object]:
    """Replace the two chemistry steps of the tree edits: `mol_from_smiles(smiles)` -> the kekulized molecule stored on an edited
    node (reference: Chem.MolFromSmiles + Chem.Kekulize), `can_assemble(node)` -> bool (generation/jtnn/jtnn_dec.py).  None
    restores the default (a lazy import of rdkit / generation.jtnn.jtnn_dec).  Returns the previous hooks."""
    prev = dict(_HOOKS)
    _HOOKS["mol_from_smiles"] = mol_from_smiles
    _HOOKS["can_assemble"] = can_assemble
    return prev


def _mol_from_smiles(smiles):
    fn = _HOOKS["mol_from_smiles"]
    if fn is None:
        try:
            from rdkit import Chem
        except ImportError as exc:
            raise ImportError("a refine tree edit needs RDKit to rebuild the edited fragment's molecule: install rdkit or call "
                              "hierdiff_amd.refine.set_chem_hooks(mol_from_smiles=...)") from exc

        def fn(s):
            mol = Chem.MolFromSmiles(s)
            Chem.Kekulize(mol)
            return mol
    return fn(smiles)


def _can_assemble(node) -> bool:
    fn = _HOOKS["can_assemble"]
    if fn is None:
        try:
            from generation.jtnn.jtnn_dec import can_assemble as fn
        except ImportError as exc:
            raise ImportError("a refine tree edit needs JT-VAE's can_assemble (generation.jtnn.jtnn_dec of the HierDiff tree): put it "
                              "on sys.path or call hierdiff_amd.refine.set_chem_hooks(can_assemble=...)") from exc
    return bool(fn(node))


def _is_exact(node) -> bool:
    return any(k.__name__ == "MolTreeNode" for k in type(node).__mro__)


# ----------------------------------------------------------------------------- host helpers (model_refine.py:306-349)
def get_bfs_depth_edges(edges, center, n_nodes):
    """Directed edges child -> parent of a breadth-first search from `center` over the edge list `edges` ([sources, targets]),
    grouped by the child's depth, deepest group first: [[children, parents], ...].  A lone node raises IndexError, as in the
    reference."""
    src, dst = list(edges[0]), list(edges[1])
    depth = [0] * n_nodes
    depth[center] = 1
    todo = deque([center])
    while todo:
        u = todo.popleft()
        for a, b in zip(src, dst):
            if a == u and depth[b] == 0:
                depth[b] = depth[u] + 1
                todo.append(b)
    groups = [[[], []] for _ in range(max(depth) - 1)]
    if len(groups[0]) == 0:                     # (never true for a list of pairs; the reference's fallback, kept)
        groups = [groups]
    for a, b in zip(src, dst):
        if depth[a] < depth[b]:
            groups[depth[b] - 2][0].append(b)
            groups[depth[b] - 2][1].append(a)
    groups.reverse()
    return groups


def flat_add_and_concat(edges, n_nodes):
    """Per-copy depth lists -> one depth list over the stacked batch: copy i's node ids move by i * n_nodes, groups of the same
    depth index are concatenated in copy order.  (The reference also shifts the ids of its argument in place; this returns new
    lists and leaves the argument as it is.)"""
    deepest = max(len(e) for e in edges)
    if deepest == 0:
        return [[[], []]]
    out = [[[], []] for _ in range(deepest)]
    for i, groups in enumerate(edges):
        shift = i * n_nodes
        for d, (rows, cols) in enumerate(groups):
            out[d][0].extend(r + shift for r in rows)
            out[d][1].extend(c + shift for c in cols)
    return out


# ----------------------------------------------------------------------------- parameters
def refine_param_shapes(vocab_size: int, feature_size: int, hidden_size: int, n_layers: int) -> "OrderedDict[str, tuple]":
    """Node2Vec parameters in the reference's registration order (model_refine.py:19-45)."""
    H = hidden_size
    s: "OrderedDict[str, tuple]" = OrderedDict()
    s["v_embedding.weight"] = (vocab_size + 1, H)
    s["f_embedding.0.weight"] = (H, feature_size); s["f_embedding.0.bias"] = (H,)
    s["f_embedding.2.weight"] = (H, H); s["f_embedding.2.bias"] = (H,)
    s["projection.0.weight"] = (3 * H, 3 * H); s["projection.0.bias"] = (3 * H,)
    s["projection.2.weight"] = (H, 3 * H); s["projection.2.bias"] = (H,)
    s["projection.4.weight"] = (H, H); s["projection.4.bias"] = (H,)
    s["size_embedding.weight"] = (N_SIZES, H)
    layer = egcl_param_shapes(H, 1, 0, attention=True, edge_update=False)
    for i in range(n_layers):
        for kind in _KINDS:
            for k, shp in layer.items():
                s[f"gcl_{kind}{i}.{k}"] = shp
    s["output.0.weight"] = (H, H + 1); s["output.0.bias"] = (H,)
    s["output.2.weight"] = (vocab_size, H); s["output.2.bias"] = (vocab_size,)
    return s


def synthetic_refine_state_dict(vocab_size: int, feature_size: int, hidden_size: int, n_layers: int, seed: int = 0,
                                coord_gain: float = 0.3) -> "OrderedDict[str, np.ndarray]":
    """Deterministic weights keyed by tensor name (the reference ships no refine checkpoint): embeddings N(0, 1) like
    nn.Embedding, Linear layers uniform(+-1/sqrt(fan_in)) like nn.Linear, E_GCL layers from stage2.synthetic_egcl_state_dict."""
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    shapes = refine_param_shapes(vocab_size, feature_size, hidden_size, n_layers)
    layers: Dict[str, "OrderedDict[str, np.ndarray]"] = {}
    for name, shape in shapes.items():
        if name.startswith("gcl_"):
            prefix, key = name.split(".", 1)
            if prefix not in layers:
                sub = int.from_bytes(hashlib.sha256(f"refine:{seed}:{prefix}".encode()).digest()[:4], "little")
                layers[prefix] = synthetic_egcl_state_dict(hidden_size, 1, 0, True, False, sub, coord_gain=coord_gain)
            out[name] = layers[prefix][key]
            continue
        digest = hashlib.sha256(f"refine:{seed}:{name}".encode()).digest()
        rng = np.random.Generator(np.random.PCG64(int.from_bytes(digest[:8], "little")))
        if name in ("v_embedding.weight", "size_embedding.weight"):
            out[name] = rng.standard_normal(shape).astype(np.float32)
        else:
            wshape = shapes[name[:-4] + "weight"] if name.endswith("bias") else shape
            bound = 1.0 / math.sqrt(wshape[1])
            out[name] = rng.uniform(-bound, bound, size=shape).astype(np.float32)
    return out


# ----------------------------------------------------------------------------- kernels
def _stream(dev: torch.device):
    return torch.cuda.current_stream(dev).cuda_stream


def _dev_index(dev: torch.device) -> int:
    return torch.cuda.current_device() if dev.index is None else int(dev.index)


def _input_forward(v, s, f, Ev, Es, W1, b1, W2, b2):
    """The projection input cat[v_embedding(v), f_embedding(f), size_embedding(s)] [M][3H] without a concat copy; also the
    device flag of an out-of-range id and the f_embedding activations the backward needs."""
    M, H = v.numel(), Ev.shape[1]
    comb = torch.empty((M, 3 * H), device=f.device, dtype=torch.float32)
    bad = torch.zeros(1, device=f.device, dtype=torch.int32)
    _lib.check(_lib.load().hd_refine_embed_forward(_dev_index(f.device), v.data_ptr(), s.data_ptr(), M, H, Ev.shape[0], Es.shape[0],
                                                   Ev.data_ptr(), Es.data_ptr(), comb.data_ptr(), comb.stride(0), 0, 2 * H,
                                                   bad.data_ptr(), _stream(f.device)), "hd_refine_embed_forward")
    pre, act = _linear_fwd(f, W1, b1, epi=_EPI_BIAS_SILU2)
    _gemm(M, H, H, act, act.stride(0), 1, W2, 1, W2.stride(0), comb[:, H:2 * H], bias=b2)
    return comb, bad, pre, act


class _InputStage(torch.autograd.Function):
    """Embedding gathers + f_embedding MLP into the projection input; backward: dEv / dEs per id in row order
    (hd_refine_embed_backward) and the f_embedding weights on hd_gemm_f32."""

    @staticmethod
    def forward(ctx, v, s, f, Ev, Es, W1, b1, W2, b2):
        Ev, Es, W1, b1, W2, b2 = (t.detach().contiguous() for t in (Ev, Es, W1, b1, W2, b2))
        comb, bad, pre, act = _input_forward(v, s, f, Ev, Es, W1, b1, W2, b2)
        ctx.save_for_backward(v, s, f, pre, act, W2)
        ctx.sizes = (Ev.shape[0], Es.shape[0])
        ctx.mark_non_differentiable(bad)
        return comb, bad

    @staticmethod
    def backward(ctx, gcomb, _gbad):
        v, s, f, pre, act, W2 = ctx.saved_tensors
        g = gcomb.detach().to(torch.float32).contiguous()
        M, H = v.numel(), W2.shape[0]
        nv, ns = ctx.sizes
        dEv = torch.empty((nv, H), device=g.device, dtype=torch.float32)
        dEs = torch.empty((ns, H), device=g.device, dtype=torch.float32)
        _lib.check(_lib.load().hd_refine_embed_backward(_dev_index(g.device), v.data_ptr(), s.data_ptr(), M, H, nv, ns, g.data_ptr(),
                                                        g.stride(0), 0, 2 * H, dEv.data_ptr(), dEs.data_ptr(), _stream(g.device)),
                   "hd_refine_embed_backward")
        g1 = g[:, H:2 * H]
        dW2, db2 = _linear_dw(g1, act, True)
        dpre = _linear_dx(g1, W2, epi=_EPI_MUL_DSILU, aux=pre)
        dW1, db1 = _linear_dw(dpre, f, True)
        return None, None, None, dEv, dEs, dW1, db1, dW2, db2


def _sqdist_value(g, x):
    ea = torch.empty((g.E, 1), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().hd_sqdist_forward(g._h, x.data_ptr(), ea.data_ptr(), _stream(x.device)), "hd_sqdist_forward")
    return ea


class _SqDist(torch.autograd.Function):
    """edge_attr = |x_row - x_col|^2 [E][1] on an E_GCL edge graph; backward: CSR sums over row and col (deterministic)."""

    @staticmethod
    def forward(ctx, g, x):
        xc = x.detach().to(torch.float32).contiguous()
        ctx.g = g
        ctx.save_for_backward(xc)
        return _sqdist_value(g, xc)

    @staticmethod
    def backward(ctx, gea):
        (xc,) = ctx.saved_tensors
        dea = gea.detach().to(torch.float32).contiguous()
        dx = torch.empty_like(xc)
        _lib.check(_lib.load().hd_sqdist_backward(ctx.g._h, xc.data_ptr(), dea.data_ptr(), dx.data_ptr(), _stream(xc.device)),
                   "hd_sqdist_backward")
        return None, dx


class CandTable:
    """Candidate sets on the device: the ids of every set back to back (int32) and per-set offsets."""

    def __init__(self, sets: Sequence[Sequence[int]], ncols: int, device):
        flat, off = [], [0]
        for cands in sets:
            cands = [int(c) for c in cands]
            if len(set(cands)) != len(cands):
                raise ValueError("a candidate set lists an id twice")
            if any(c < 0 or c >= ncols for c in cands):
                raise ValueError(f"a candidate id is outside the {ncols} output columns")
            flat.extend(cands)
            off.append(len(flat))
        self.nsets, self.ncols = len(sets), ncols
        self.ids = torch.tensor(flat if flat else [0], dtype=torch.int32, device=device)
        self.off = torch.tensor(off, dtype=torch.int32, device=device)


def cand_xent_forward(logits, table: CandTable, set_idx, target, k, logp, hit, topk, err):
    """hd_cand_xent_forward on device tensors (set_idx / target int32 [B]; logp float [B]; hit int32 [B]; topk int32 [B][k];
    err int32 [1], zeroed by the caller)."""
    _lib.check(_lib.load().hd_cand_xent_forward(_dev_index(logits.device), logits.shape[0], logits.data_ptr(), logits.stride(0),
                                                table.ncols, table.ids.data_ptr(), table.off.data_ptr(), table.nsets,
                                                set_idx.data_ptr(), target.data_ptr(), k, logp.data_ptr(), hit.data_ptr(),
                                                topk.data_ptr() if k > 0 else None, err.data_ptr(), _stream(logits.device)),
               "hd_cand_xent_forward")


class CandXent(torch.autograd.Function):
    """(logp [B], flags [B + 1] = hit | err) = the size-restricted softmax head; logp is differentiable with respect to the logits."""

    @staticmethod
    def forward(ctx, logits, table, set_idx, target):
        lg = logits.detach().to(torch.float32).contiguous()
        B = lg.shape[0]
        logp = torch.empty(B, device=lg.device, dtype=torch.float32)
        flags = torch.zeros(B + 1, device=lg.device, dtype=torch.int32)
        cand_xent_forward(lg, table, set_idx, target, 0, logp, flags[:B], None, flags[B:])
        ctx.table = table
        ctx.save_for_backward(lg, set_idx, target)
        ctx.mark_non_differentiable(flags)
        return logp, flags

    @staticmethod
    def backward(ctx, glogp, _gflags):
        lg, set_idx, target = ctx.saved_tensors
        t = ctx.table
        dloss = (-glogp).detach().to(torch.float32).contiguous()
        dlogits = torch.zeros_like(lg) if lg.shape[1] != t.ncols else torch.empty_like(lg)
        _lib.check(_lib.load().hd_cand_xent_backward(_dev_index(lg.device), lg.shape[0], lg.data_ptr(), lg.stride(0), t.ncols,
                                                     t.ids.data_ptr(), t.off.data_ptr(), t.nsets, set_idx.data_ptr(),
                                                     target.data_ptr(), dloss.data_ptr(), dlogits.data_ptr(), _stream(lg.device)),
                   "hd_cand_xent_backward")
        return dlogits, None, None, None


# ----------------------------------------------------------------------------- the model
class Node2Vec(nn.Module):
    """HIP implementation of models/model_refine.py:Node2Vec."""

    def __init__(self, size_dict, vocab_size, feature_size, hidden_size, n_layers=3):
        super().__init__()
        if isinstance(size_dict, (str, bytes, os.PathLike)):
            with open(size_dict, "rb") as fh:
                size_dict = pickle.load(fh)
        self.size_dict = {int(k): [int(i) for i in v] for k, v in dict(size_dict).items()}
        self.feature_size = feature_size
        self.vocab_size = vocab_size
        H = hidden_size
        self.v_embedding = nn.Embedding(vocab_size + 1, H)
        self.f_embedding = nn.Sequential(nn.Linear(feature_size, H), nn.SiLU(), nn.Linear(H, H))
        self.projection = nn.Sequential(nn.Linear(3 * H, 3 * H), nn.SiLU(), nn.Linear(3 * H, H), nn.SiLU(), nn.Linear(H, H))
        self.size_embedding = nn.Embedding(N_SIZES, H)
        self.n_layers = n_layers
        for i in range(n_layers):
            for kind in _KINDS:
                self.add_module(f"gcl_{kind}{i}", E_GCL(H, H, H, edges_in_d=1, act_fn=nn.SiLU(), recurrent=True, attention=True,
                                                        tanh=True, coords_range=30, agg='sum', coord_update=True, edge_update=False))
        self.output = nn.Sequential(nn.Linear(H + 1, H), nn.SiLU(), nn.Linear(H, vocab_size))
        self._tables: Dict[tuple, CandTable] = {}

    # ------------------------------------------------------------------ plumbing
    def _device(self) -> torch.device:
        dev = self.v_embedding.weight.device
        if dev.type != "cuda":
            raise HierDiffHipError("Node2Vec runs only on an MI355X: move the module to a cuda device (there is no CPU fallback)")
        _lib.require_gpu()
        return dev

    def _layers_frozen(self, on: bool):
        """Parameters do not change inside one call: the E_GCL layers confirm their packed weights once per call."""
        for m in self.modules():
            if isinstance(m, E_GCL):
                if on:
                    m._frozen = False
                    m._sync_weights()
                m._frozen = on

    def _table(self, sets: List[List[int]], dev: torch.device) -> CandTable:
        key = (str(dev), tuple(tuple(c) for c in sets))
        t = self._tables.get(key)
        if t is None:
            if len(self._tables) >= 32:
                self._tables.pop(next(iter(self._tables)))
            t = CandTable(sets, self.vocab_size, dev)
            self._tables[key] = t
        return t

    def _check_ids(self, v: np.ndarray, size: np.ndarray):
        """nn.Embedding's range check, on the host before any launch."""
        if v.size and (v.min() < 0 or v.max() > self.vocab_size):
            raise IndexError(f"node vocabulary id out of range for v_embedding ({self.vocab_size + 1} rows)")
        if size.size and (size.min() < 0 or size.max() >= N_SIZES):
            raise IndexError(f"node size out of range for size_embedding ({N_SIZES} rows: sizes 0..{N_SIZES - 1})")

    def _dense(self, x, layer: nn.Linear, silu: bool, grad: bool):
        if grad:
            y = _Linear.apply(x, layer.weight, layer.bias)
            return F.silu(y) if silu else y
        W, b = layer.weight.detach().contiguous(), layer.bias.detach().contiguous()
        if silu:
            return _linear_fwd(x, W, b, epi=_EPI_BIAS_SILU2)[1]
        return _linear_fwd(x, W, b)

    def _embed(self, v, s, f, grad: bool):
        """projection(cat[v_embedding(v), f_embedding(f), size_embedding(s)]) [M][H] and the device flag of bad ids."""
        fe, pr = self.f_embedding, self.projection
        args = (v, s, f, self.v_embedding.weight, self.size_embedding.weight, fe[0].weight, fe[0].bias, fe[2].weight, fe[2].bias)
        if grad:
            comb, bad = _InputStage.apply(*args)
        else:
            comb, bad, _, _ = _input_forward(*(a.detach().contiguous() for a in args))
        h = self._dense(comb, pr[0], True, grad)
        h = self._dense(h, pr[2], True, grad)
        return self._dense(h, pr[4], False, grad), bad

    def _head(self, h, rows, val, grad: bool):
        z = torch.cat([h.index_select(0, rows), val.to(h.device, torch.float32).reshape(-1, 1)], dim=1)
        return self._dense(self._dense(z, self.output[0], True, grad), self.output[2], False, grad)

    def message(self, edges, h, x, mask=None):
        """model_refine.py:47-69: three passes over the per-depth edge lists (collect, reverse with row / col swapped, back); every
        depth runs all n_layers layers of its pass, each after recomputing edge_attr = |x_row - x_col|^2."""
        reverse = [[cols, rows] for rows, cols in reversed(list(edges))]
        for kind, levels in (("collect", edges), ("reverse", reverse), ("back", edges)):
            for rows, cols in levels:
                if len(rows) == 0:
                    raise ValueError("an empty per-depth edge list ([[], []]) is not defined (the reference fails on it too)")
                row = torch.as_tensor(list(rows), dtype=torch.int32)
                col = torch.as_tensor(list(cols), dtype=torch.int32)
                for i in range(self.n_layers):
                    layer = self._modules[f"gcl_{kind}{i}"]
                    g = layer._graph(row, col, h.shape[0])
                    ea = _SqDist.apply(g, x) if x.requires_grad else _sqdist_value(g, x.detach().contiguous())
                    h, x = layer(h, [row, col], x, edge_attr=ea, node_mask=mask)
        return h, x

    # ------------------------------------------------------------------ reference API
    def forward(self, batch):
        """model_refine.py:71-111 on PadCollate's dict -> {'loss': sum of per-sample cross-entropies over the predicted
        fragment's candidate set, 'accuracy': fraction whose argmax over the set is the label}."""
        f, v, size, x = batch['feature'], batch['vocab'], batch['size'], batch['pos']
        edges, mask, label, predict_idx, val = batch['edges'], batch['mask'], batch['label'], batch['predict_idx'], batch['val']
        bs, n = f.shape[:2]
        M = bs * n
        v_h = v.detach().reshape(-1).cpu().numpy()
        s_h = size.detach().reshape(-1).cpu().numpy()
        self._check_ids(v_h, s_h)
        rows_h = [i * n + int(p) for i, p in enumerate(predict_idx)]
        psize = [int(s_h[r]) for r in rows_h]
        labels = [int(t) for t in label.reshape(-1).tolist()]
        keys = sorted(set(psize))
        sets = [self.size_dict[k] for k in keys]                       # KeyError for a size without an entry, as the reference
        for k, t in zip(psize, labels):
            self.size_dict[k].index(t)                                  # ValueError: a label outside its candidate set
        dev = self._device()
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        table = self._table(sets, dev)
        set_idx = torch.tensor([keys.index(k) for k in psize], dtype=torch.int32).to(dev)
        target = torch.tensor(labels, dtype=torch.int32).to(dev)
        rows = torch.tensor(rows_h, dtype=torch.int64).to(dev)
        vd = torch.from_numpy(v_h.astype(np.int64)).to(dev)
        sd = torch.from_numpy(s_h.astype(np.int64)).to(dev)
        fd = f.detach().to(dev, torch.float32).reshape(M, -1).contiguous()
        xd = x.detach().to(dev, torch.float32).reshape(M, -1).contiguous()
        md = mask.detach().to(dev, torch.float32).reshape(M, -1).contiguous()
        self._layers_frozen(True)
        try:
            h, bad = self._embed(vd, sd, fd, grad)
            h = h * md
            h, xd = self.message(edges, h, xd, md)
            logits = self._head(h, rows, val, grad)
            if grad:
                logp, flags = CandXent.apply(logits, table, set_idx, target)
            else:
                logp = torch.empty(bs, device=dev, dtype=torch.float32)
                flags = torch.zeros(bs + 1, device=dev, dtype=torch.int32)
                cand_xent_forward(logits.contiguous(), table, set_idx, target, 0, logp, flags[:bs], None, flags[bs:])
        finally:
            self._layers_frozen(False)
        chk = torch.cat([bad, flags[bs:]]).cpu()
        if int(chk[0]):
            raise IndexError("a node vocabulary id or size is out of range for its embedding")
        if int(chk[1]):
            raise ValueError("a label is not in its candidate set")
        return {'loss': -logp.sum(), 'accuracy': flags[:bs].to(torch.float32).sum() / bs}

    @torch.no_grad()
    def check_node(self, vocab, nodes, edges, pad_idx, pad_wid, device=None, check_num=1):
        """model_refine.py:114-172: one copy of the tree per entry of pad_idx with that node masked (v = 780); per copy
        (log-softmax over the candidates of the node's size at pad_wid, top check_num candidates with "== pad_wid" flags) -
        a tuple (flag, id) when check_num is 1, a list of them otherwise.  One device -> host copy of the results per call.
        (`device` is kept for the reference's signature; the module's own device is used.)"""
        bs, n = len(pad_idx), len(nodes)
        if check_num > MAX_TOPK:
            raise NotImplementedError(f"check_num > {MAX_TOPK}")
        pos = np.asarray([np.asarray(nd.pos, dtype=np.float32).reshape(3) for nd in nodes], dtype=np.float32)
        fp = np.asarray([np.asarray(nd.fp[:self.feature_size], dtype=np.float32) for nd in nodes], dtype=np.float32)
        wid = np.asarray([int(nd.wid) for nd in nodes], dtype=np.int64)
        sizes = np.asarray([int(nd.size) for nd in nodes], dtype=np.int64)
        v_all = np.tile(wid, bs)
        for i, p in enumerate(pad_idx):
            v_all[i * n + int(p)] = MASK_TOKEN
        self._check_ids(v_all, sizes)
        cand, ks, targets = [], [], []
        k = check_num
        for i in range(bs):
            c = [int(t) for t in vocab.get_size(nodes[pad_idx[i]].size)]
            if len(c) == 0:
                raise TypeError(f"no candidate fragment of size {nodes[pad_idx[i]].size}: the reference reaches "
                                "handle_wrong_sizes(size) without its vocab argument here")
            if len(c) < k:
                k = len(c)                                  # shrinks for every later row too (reference quirk)
            ks.append(k)
            targets.append(c[c.index(int(pad_wid[i]))])     # ValueError: pad_wid outside the candidate set
            cand.append(c)
        keys: List[List[int]] = []
        for c in cand:
            if c not in keys:
                keys.append(c)
        val = [sum(1 for a in edges[0] if a == pad_idx[i]) for i in range(bs)]
        depth_edges = flat_add_and_concat([get_bfs_depth_edges(edges, pad_idx[i], n) for i in range(bs)], n)
        dev = self._device()
        table = self._table(keys, dev)
        kk = max(0, check_num)
        M = bs * n
        ids = torch.from_numpy(np.concatenate([v_all, np.tile(sizes, bs), [keys.index(c) for c in cand], targets,
                                               [i * n + int(p) for i, p in enumerate(pad_idx)]]).astype(np.int64)).to(dev)
        flt = torch.from_numpy(np.concatenate([np.tile(fp, (bs, 1)).reshape(-1), np.tile(pos, (bs, 1)).reshape(-1),
                                               np.asarray(val, dtype=np.float32)]).astype(np.float32)).to(dev)
        fd = flt[:M * self.feature_size].view(M, self.feature_size)
        xd = flt[M * self.feature_size:M * (self.feature_size + 3)].view(M, 3)
        vald = flt[M * (self.feature_size + 3):]
        meta = ids[2 * M:].view(3, bs)
        res = torch.zeros(bs * (2 + kk) + 2, dtype=torch.int32, device=dev)      # logp | hit | topk | bad | err
        self._layers_frozen(True)
        try:
            h, bad = self._embed(ids[:M], ids[M:2 * M], fd, False)
            h, xd = self.message(depth_edges, h, xd)
            logits = self._head(h, meta[2], vald, False).contiguous()
            cand_xent_forward(logits, table, meta[0].to(torch.int32), meta[1].to(torch.int32), kk, res[:bs].view(torch.float32),
                              res[bs:2 * bs], res[2 * bs:2 * bs + bs * kk].view(bs, kk), res[-1:])
            res[-2:-1].copy_(bad)
        finally:
            self._layers_frozen(False)
        out = res.cpu()
        if int(out[-2]) or int(out[-1]):
            raise HierDiffHipError("check_node: the device reported an out-of-range id or a pad_wid outside its set")
        logp = out[:bs].view(torch.float32)
        top = out[2 * bs:2 * bs + bs * kk].view(bs, kk)
        results = []
        for i in range(bs):
            best = [int(t) for t in top[i, :ks[i]]]
            if ks[i] == 1:
                results.append((logp[i].clone(), (best[0] == pad_wid[i], best[0])))
            else:
                results.append((logp[i].clone(), [(p == pad_wid[i], p) for p in best]))
        return results

    def check_tree(self, beam_tree, vocab, device=None, check_num=0.1):
        """model_refine.py:174-247: score every exact node of the tree; among the lowest-scoring ones (at most check_num of them,
        in the first half of the node order) try the first whose top candidate is not its own fragment; keep that edit if the
        tree's summed log-probability rises and the node and its neighbours still assemble.  Returns (beam_tree, pertube_p_sum,
        edited)."""
        tree = beam_tree.tree
        edges = _adjacency_edges(tree.adj_matrix)
        nodes_exact = [nd for nd in tree.nodes if _is_exact(nd)]
        if len(nodes_exact) * check_num <= 1:
            return beam_tree, 0.0, False
        to_exact = {}
        for i, nd in enumerate(tree.nodes):
            if _is_exact(nd):
                to_exact[i] = len(to_exact)
        to_tree = {e: i for i, e in to_exact.items()}
        edges = [[to_exact[a] for a in edges[0]], [to_exact[b] for b in edges[1]]]
        everyone = list(range(len(nodes_exact)))
        scored = self.check_node(vocab, nodes_exact, edges, everyone, [nd.wid for nd in nodes_exact], device)
        p = torch.tensor([r[0] for r in scored])
        sum_p = torch.sum(p)
        order = torch.argsort(p)
        limit = int(len(nodes_exact) * check_num)
        if order.shape[0] > limit:
            order = order[:limit]
        order = [int(i) for i in order if i < len(nodes_exact) * 0.5]
        for i in order:
            if scored[i][1][0]:
                continue
            new_wid = scored[i][1][1]
            trial = copy.deepcopy(nodes_exact)
            _retype(trial[i], new_wid, vocab)
            rescored = self.check_node(vocab, trial, edges, everyone, [nd.wid for nd in trial], device)
            p_new = torch.sum(torch.tensor([r[0] for r in rescored]))
            group = [trial[i]] + trial[i].neighbors
            assembles = sum(_can_assemble(nd) for nd in group) == len(group)
            if p_new > sum_p and assembles:
                target = tree.nodes[to_tree[i]]
                _retype(target, new_wid, vocab)
                tree.nodes[to_tree[i]] = target
                beam_tree.tree = tree
                return beam_tree, -p_new.item() + sum_p.item(), True
        beam_tree.tree = tree
        return beam_tree, 0.0, False

    def check_final_tree(self, beam_tree, vocab, device=None, check_num=10):
        """model_refine.py:250-302: the nodes that cannot be assembled are re-scored; each is replaced by the first of its top
        check_num candidates that assembles and raises the tree's summed log-probability.  Returns the tree when every such node
        was corrected (or none needed it); None otherwise, or when more than a fifth of the nodes fail."""
        tree = beam_tree.tree
        edges = _adjacency_edges(tree.adj_matrix)
        broken = [i for i in range(len(tree.nodes)) if not _can_assemble(tree.nodes[i])]
        if len(broken) == 0:
            return beam_tree
        if len(broken) > 0.2 * len(tree.nodes):
            return None
        corrected = 0
        scored = self.check_node(vocab, tree.nodes, edges, broken, [tree.nodes[i].wid for i in broken], device, check_num)
        sum_p = torch.sum(torch.tensor([r[0] for r in scored]))
        for i, result in enumerate(scored):
            options = result[1] if isinstance(result[1], list) else [result[1]]
            for j in range(min(check_num, len(options))):
                if options[j][0]:
                    continue
                idx = broken[i]
                trial = copy.deepcopy(tree.nodes)
                _retype(trial[idx], options[j][1], vocab)
                everyone = list(range(len(trial)))
                rescored = self.check_node(vocab, trial, edges, everyone, [nd.wid for nd in trial], device)
                p_new = torch.sum(torch.tensor([r[0] for r in rescored]))
                if _can_assemble(trial[idx]) and p_new > sum_p:
                    tree.nodes = trial
                    beam_tree.tree = tree
                    corrected += 1
                    break
        return beam_tree if corrected == len(broken) else None


def _adjacency_edges(adj):
    """[sources, targets] of the nonzero entries of an adjacency matrix, in row-major order."""
    nz = torch.as_tensor(np.asarray(adj)).nonzero()
    return [nz[:, 0].tolist(), nz[:, 1].tolist()]


def _retype(node, wid, vocab):
    """Give a tree node another fragment: id, SMILES and molecule (model_refine.py:200-205)."""
    node.wid = wid
    node.smiles = vocab.get_smiles(wid)
    node.mol = _mol_from_smiles(node.smiles)
