"""MI355X drop-in for the reference's ``nn.state2state.egnn_aether.EGNN_vel_Aether`` (the model
experiments/lorentz/main.py:147 builds for ``--model egnn_aether``).

Same constructor, ``forward(h, x, edges, vel, edge_attr, charges)`` signature and ``state_dict`` keys / shapes / order
(egnn_aether.py:12-56, gcl.py:8-50, egnn/gcl.py:17-51), and the same default initialisation under a torch seed.  The
computation runs in ``libaether_hip.so`` (``aether_egnn_forward`` / ``aether_egnn_backward``, csrc/egnn.h); there is no
PyTorch or CPU fallback.  With gradients enabled the step goes through ``_paramgrad._ParamGradStep``: parameter gradients
only, written into one flat buffer (the runner detaches every input, main.py:254-259), so ``GraphedTrainStep``,
``FusedAdamW`` and ``attach_data_parallel`` work as they do for ``Aether``.  The plumbing around the library calls is
``_paramgrad.ParamGradModule``'s.

One difference, on purpose: the reference adds into the caller's ``x`` in place (egnn/gcl.py:97, gcl.py:81); this module
returns a new tensor and leaves ``x`` as it was.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ... import _lib
from ._paramgrad import ParamGradModule
from .aether import _FieldNetwork

SUPPORTED_HIDDEN = (64, 128)


class E_GCL_vel_field(nn.Module):
    """Parameter holder with the reference's names; construction order as egnn/gcl.py:17-51 + gcl.py:16-48, so that
    the default initialisation under a torch seed is the reference's (phi's last Linear is created and initialised with
    xavier gain 0.001 BEFORE coord_mlp[0])."""

    def __init__(self, hidden_nf, edges_in_d, num_dims, tanh):
        super().__init__()
        act = nn.SiLU()
        self.edge_mlp = nn.Sequential(nn.Linear(2 * hidden_nf + 1 + edges_in_d, hidden_nf), act,
                                      nn.Linear(hidden_nf, hidden_nf), act)
        self.node_mlp = nn.Sequential(nn.Linear(2 * hidden_nf, hidden_nf), act, nn.Linear(hidden_nf, hidden_nf))
        layer = nn.Linear(hidden_nf, 1, bias=False)
        torch.nn.init.xavier_uniform_(layer.weight, gain=0.001)
        coord_mlp = [nn.Linear(hidden_nf, hidden_nf), act, layer]
        if tanh:
            coord_mlp.append(nn.Tanh())
        self.coord_mlp = nn.Sequential(*coord_mlp)
        self.coord_mlp_vel = nn.Sequential(nn.Linear(hidden_nf + num_dims, hidden_nf), act, nn.Linear(hidden_nf, 1))


class EGNN_vel_Aether(ParamGradModule):
    """Drop-in for nn/state2state/egnn_aether.py:12-75."""
    NAME = "EGNN_vel_Aether"
    ENTRY = "aether_egnn"
    KEEP = _lib.EGNN_KEEP

    def __init__(self, in_node_nf, in_edge_nf, hidden_nf, num_dims=3, device="cpu", act_fn=nn.SiLU(), n_layers=4,
                 coords_weight=1.0, recurrent=False, norm_diff=False, tanh=False):
        super().__init__()
        if num_dims != 3:
            raise ValueError("EGNN_vel_Aether: num_dims must be 3 (the field net and the kernels are 3-D)")
        if hidden_nf not in SUPPORTED_HIDDEN:
            raise ValueError(f"EGNN_vel_Aether: hidden_nf must be one of {SUPPORTED_HIDDEN}")
        if not (1 <= int(n_layers) <= 64):
            raise ValueError("EGNN_vel_Aether: n_layers must lie in [1, 64]")
        if not (1 <= int(in_node_nf) <= 4096):
            raise ValueError("EGNN_vel_Aether: in_node_nf must lie in [1, 4096]")
        if in_edge_nf != 2 + 2 * num_dims:
            raise ValueError("EGNN_vel_Aether: in_edge_nf must be 8 (edge_attr [q_i q_j, |x_i - x_j|^2] + the field at "
                             "both ends, experiments/lorentz/main.py:147,254-259)")
        if not recurrent:
            raise ValueError("EGNN_vel_Aether: only recurrent=True is supported (the runner's setting)")
        if float(coords_weight) != 1.0:
            raise ValueError("EGNN_vel_Aether: only coords_weight=1 is supported")
        if type(act_fn) is not nn.SiLU:
            raise ValueError("EGNN_vel_Aether: only act_fn=nn.SiLU() is supported")
        self.hidden_nf = int(hidden_nf)
        self.in_node_nf = int(in_node_nf)
        self.device = device
        self.n_layers = int(n_layers)
        self.num_dims = num_dims
        self.norm_diff = bool(norm_diff)
        self.tanh = bool(tanh)
        self.embedding = nn.Linear(in_node_nf, self.hidden_nf)
        for i in range(self.n_layers):
            self.add_module("gcl_%d" % i, E_GCL_vel_field(self.hidden_nf, in_edge_nf, num_dims, self.tanh))
        self.field_net = _FieldNetwork(num_dims, 32, 16)
        self._flags = (_lib.EGNN_NORM_DIFF if self.norm_diff else 0) | (_lib.EGNN_TANH if self.tanh else 0)
        self._finish_init()

    def _sizes(self):
        return self.hidden_nf, self.n_layers, self.in_node_nf

    def _inputs(self, h, x, edges, vel, edge_attr, charges):
        if not x.is_cuda:
            raise _lib.AetherHipError("aether_amd EGNN_vel_Aether runs on an MI355X only; got a CPU tensor "
                                      "(there is no CPU fallback)")
        if torch.is_grad_enabled() and any(t.requires_grad for t in (h, x, vel, edge_attr, charges)):
            raise _lib.AetherHipError("EGNN_vel_Aether: gradients flow to the parameters only (the runner detaches every "
                                      "input, experiments/lorentz/main.py:254-259); detach the inputs")
        row, col = edges
        if row.dtype != torch.int64 or col.dtype != torch.int64:
            raise TypeError("edges must be int64 (torch.LongTensor), as in the reference")
        n_nodes = x.shape[0]
        E = row.numel()
        if x.shape != (n_nodes, 3) or vel.shape != x.shape:
            raise ValueError("x / vel must be [n_nodes, 3]")
        if h.shape != (n_nodes, self.in_node_nf) or col.numel() != E or edge_attr.shape != (E, 2) or \
                charges.numel() != n_nodes:
            raise ValueError("h / edge index / edge_attr / charges shapes do not match")
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        graph = self.prepare_graph((row, col), n_nodes)
        return f32(h), f32(x), f32(vel), (f32(edge_attr), f32(charges)), (), graph

    # -- reference surface -----------------------------------------------------------
    def forward(self, h, x, edges, vel, edge_attr, charges):
        return self._run(*self._inputs(h, x, edges, vel, edge_attr, charges))

    # -- test hook -------------------------------------------------------------------
    @torch.no_grad()
    def forward_layers(self, h, x, edges, vel, edge_attr, charges):
        """(out, [h_0 .. h_L], [x_0 .. x_L]): every layer's input h / x (the embedding's output, then each layer's), from
        a keep-for-backward forward."""
        return self._run_layers(*self._inputs(h, x, edges, vel, edge_attr, charges))
