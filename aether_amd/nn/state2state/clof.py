"""MI355X drop-ins for the reference's ``nn.state2state.clof.clof.{ClofNet, ClofNet_vel, ClofNet_vel_gbf}`` (the models
experiments/lorentz/main.py:152-157 builds for ``--model clof``, ``clof_vel`` and ``clof_vel_gbf``).

Same constructors, ``forward(h, x, edges, vel, edge_attr, node_attr=None, n_nodes=5)`` signature and ``state_dict`` keys /
shapes / order (clof.py, clof/gcl.py, clof/layers.py, egnn/gcl.py:17-51), and the same default initialisation under a
torch seed.  The computation runs in ``libaether_hip.so`` (``aether_clof_forward`` / ``aether_clof_backward``,
csrc/clof.h); there is no PyTorch or CPU fallback.  With gradients enabled the step goes through
``_paramgrad._ParamGradStep``: parameter gradients only, written into one flat buffer (the runner detaches every input,
main.py:266-271), so ``GraphedTrainStep``, ``FusedAdamW`` and ``attach_data_parallel`` work as they do for ``Aether``.  The
plumbing around the library calls is ``_paramgrad.ParamGradModule``'s.  Parameters that do not reach the output --
the last layer's ``node_mlp`` and ``layer_norm``, ClofNet's ``embedding_edge`` -- keep ``.grad`` None, as in the
reference, so no optimizer touches them.

Differences, on purpose: the reference adds into its centred copy of x in place, this module never writes the caller's
x; the cross products are always per edge (``torch.cross`` without ``dim`` crosses along the edge axis when there are
exactly 3 edges); the Gaussian layer's edge type is clamped to [0, 7] (the reference raises an index error outside it).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ... import _lib
from ._paramgrad import ParamGradModule

SUPPORTED_HIDDEN = (64, 128)
_HEAD = {0: 8, 1: 6, 2: 10}           # tensors before gcl_0 (include/aether_hip.h)
_PER_LAYER = 19


class Clof_GCL(nn.Module):
    """Parameter holder with the reference's names; construction order as egnn/gcl.py:17-51 then clof/gcl.py:13-24, so
    that the default initialisation under a torch seed is the reference's: E_GCL builds a two-layer edge_mlp (its random
    numbers are used up, the module is then replaced in place by Clof_GCL's three-layer one), node_mlp, the xavier-gain-0.001
    basis layer, coord_mlp.0, then coord_mlp_vel, the new edge_mlp and layer_norm."""

    def __init__(self, hidden_nf, edges_in_d, tanh):
        super().__init__()
        act = nn.SiLU()
        H = hidden_nf
        kin = 2 * H + 1 + edges_in_d
        self.edge_mlp = nn.Sequential(nn.Linear(kin, H), act, nn.Linear(H, H), act)
        self.node_mlp = nn.Sequential(nn.Linear(2 * H, H), act, nn.Linear(H, H))
        layer = nn.Linear(H, 3, bias=False)
        torch.nn.init.xavier_uniform_(layer.weight, gain=0.001)
        coord_mlp = [nn.Linear(H, H), act, layer]
        if tanh:
            coord_mlp.append(nn.Tanh())
        self.coord_mlp = nn.Sequential(*coord_mlp)
        self.coord_mlp_vel = nn.Sequential(nn.Linear(H, H), act, nn.Linear(H, 1))
        self.edge_mlp = nn.Sequential(nn.Linear(kin, H), act, nn.Linear(H, H), act, nn.Linear(H, H), act)
        self.layer_norm = nn.LayerNorm(H)


class GaussianLayer(nn.Module):
    """clof/layers.py:GaussianLayer's parameters and initialisation (K = hidden_nf / 2, 8 edge types)."""

    def __init__(self, K, edge_types=8):
        super().__init__()
        self.K = K
        self.means = nn.Embedding(1, K)
        self.stds = nn.Embedding(1, K)
        self.mul = nn.Embedding(edge_types, 1)
        self.bias = nn.Embedding(edge_types, 1)
        nn.init.uniform_(self.means.weight, 0, 3)
        nn.init.uniform_(self.stds.weight, 0, 3)
        nn.init.constant_(self.bias.weight, 0)
        nn.init.constant_(self.mul.weight, 1)


class _ClofBase(ParamGradModule):
    VARIANT = None
    ENTRY = "aether_clof"
    KEEP = _lib.CLOF_KEEP

    def __init__(self, in_node_nf, in_edge_nf, hidden_nf, device="cpu", act_fn=nn.SiLU(), n_layers=4, coords_weight=1.0,
                 recurrent=True, norm_diff=True, tanh=False):
        super().__init__()
        name = self.NAME
        if hidden_nf not in SUPPORTED_HIDDEN:
            raise ValueError(f"{name}: hidden_nf must be one of {SUPPORTED_HIDDEN}")
        if not (1 <= int(n_layers) <= 64):
            raise ValueError(f"{name}: n_layers must lie in [1, 64]")
        if not (1 <= int(in_node_nf) <= 4096):
            raise ValueError(f"{name}: in_node_nf must lie in [1, 4096]")
        if in_edge_nf != 2:
            raise ValueError(f"{name}: in_edge_nf must be 2 (edge_attr [q_i q_j, |x_i - x_j|^2], "
                             "experiments/lorentz/main.py:152-157,266-271)")
        if type(act_fn) is not nn.SiLU:
            raise ValueError(f"{name}: only act_fn=nn.SiLU() is supported")
        self.hidden_nf = int(hidden_nf)
        self.in_node_nf = int(in_node_nf)
        self.device = device
        self.n_layers = int(n_layers)
        self.coords_weight = float(coords_weight)
        self.recurrent = bool(recurrent)
        self.tanh = bool(tanh)
        self._layer_norm_diff = bool(norm_diff)
        self._variant = self.VARIANT
        H, H2 = self.hidden_nf, self.hidden_nf // 2
        self.embedding_node = nn.Linear(in_node_nf, H)
        if self.VARIANT == 0:
            self.embedding_edge = nn.Sequential(nn.Linear(in_edge_nf, 8), nn.SiLU())
        if self.VARIANT == 2:
            self.gbf = GaussianLayer(K=H2, edge_types=8)
        fuse_in = {0: 10, 1: 16, 2: 14}[self.VARIANT]
        self.fuse_edge = nn.Sequential(nn.Linear(fuse_in, H2), nn.SiLU(), nn.Linear(H2, H2), nn.SiLU())
        # ClofNet scalarizes with norm_diff; the _vel variants always normalise there (clof.py:113,190)
        self.norm_diff = bool(norm_diff) if self.VARIANT == 0 else True
        for i in range(self.n_layers):
            self.add_module("gcl_%d" % i, Clof_GCL(H, H2, self.tanh))
        self._flags = ((_lib.CLOF_NORM_DIFF if self._layer_norm_diff else 0) | (_lib.CLOF_TANH if self.tanh else 0) |
                       (_lib.CLOF_RECURRENT if self.recurrent else 0))
        self._finish_init()

    def _sizes(self):
        return self._variant, self.hidden_nf, self.n_layers, self.in_node_nf

    def _dead(self):
        """Indices (named_parameters order) of the tensors that do not reach the output: the last layer's node_mlp and
        layer_norm, ClofNet's embedding_edge.  Their .grad stays None."""
        last = _HEAD[self._variant] + _PER_LAYER * (self.n_layers - 1)
        dead = {last + 6, last + 7, last + 8, last + 9, last + 17, last + 18}
        if self._variant == 0:
            dead |= {2, 3}
        return dead

    def _inputs(self, h, x, edges, vel, edge_attr, node_attr, n_nodes):
        if node_attr is not None:
            raise ValueError(f"{self.NAME}: node_attr must be None (Clof_GCL's node_mlp has no columns for it)")
        n_per = int(n_nodes)
        if n_per < 1 or x.shape[0] % n_per != 0:
            raise ValueError(f"{self.NAME}: the node count {x.shape[0]} is not a multiple of n_nodes={n_nodes}")
        if not x.is_cuda:
            raise _lib.AetherHipError(f"aether_amd {self.NAME} runs on an MI355X only; got a CPU tensor "
                                      "(there is no CPU fallback)")
        if torch.is_grad_enabled() and any(t.requires_grad for t in (h, x, vel, edge_attr)):
            raise _lib.AetherHipError(f"{self.NAME}: gradients flow to the parameters only (the runner detaches every "
                                      "input, experiments/lorentz/main.py:266-271); detach the inputs")
        row, col = edges
        if row.dtype != torch.int64 or col.dtype != torch.int64:
            raise TypeError("edges must be int64 (torch.LongTensor), as in the reference")
        N = x.shape[0]
        E = row.numel()
        if x.shape != (N, 3) or vel.shape != x.shape:
            raise ValueError("x / vel must be [n_nodes, 3]")
        if h.shape != (N, self.in_node_nf) or col.numel() != E or edge_attr.shape != (E, 2):
            raise ValueError("h / edge index / edge_attr shapes do not match")
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        graph = self.prepare_graph((row, col), N)
        return f32(h), f32(x), f32(vel), (f32(edge_attr),), (self.coords_weight, n_per), graph

    def _rollout_call(self, n_total, n_nodes=5):
        """``rollout(x, vel, edges, charges, steps, dt=1.0, n_nodes=5)``: the forward's n_nodes.  The charges only form
        the charge product the runner puts in edge_attr[:, 0] (the forward takes none)."""
        n_per = int(n_nodes)
        if n_per < 1 or n_total % n_per != 0:
            raise ValueError(f"{self.NAME}: the node count {n_total} is not a multiple of n_nodes={n_nodes}")
        return self.coords_weight, n_per

    # -- reference surface -----------------------------------------------------------
    def forward(self, h, x, edges, vel, edge_attr, node_attr=None, n_nodes=5):
        return self._run(*self._inputs(h, x, edges, vel, edge_attr, node_attr, n_nodes))

    # -- test hook -------------------------------------------------------------------
    @torch.no_grad()
    def forward_layers(self, h, x, edges, vel, edge_attr, node_attr=None, n_nodes=5):
        """(out, [h_0 .. h_L], [x_0 .. x_L]): every layer's input h and centred x (the embedding's output and the
        centred input, then each layer's output), from a keep-for-backward forward."""
        return self._run_layers(*self._inputs(h, x, edges, vel, edge_attr, node_attr, n_nodes))


class ClofNet(_ClofBase):
    """Drop-in for nn/state2state/clof/clof.py:ClofNet (``--model clof``)."""
    VARIANT = 0
    NAME = "ClofNet"


class ClofNet_vel(_ClofBase):
    """Drop-in for nn/state2state/clof/clof.py:ClofNet_vel (``--model clof_vel``)."""
    VARIANT = 1
    NAME = "ClofNet_vel"


class ClofNet_vel_gbf(_ClofBase):
    """Drop-in for nn/state2state/clof/clof.py:ClofNet_vel_gbf (``--model clof_vel_gbf``)."""
    VARIANT = 2
    NAME = "ClofNet_vel_gbf"
