"""The Lorentz runner's data set, generated and kept on the device.

``SimulatedNBodyDataset`` has the surface of ``NBodyDataset`` (experiments/lorentz/dataset4newton.py:7-94) -- ``__len__``,
``__getitem__`` = (loc[frame_0], vel[frame_0], edge_attr, charges, loc[frame_T]), ``get_n_nodes``, ``get_edges`` -- but
instead of loading the ``loc_/vel_/edges_/charges_*.npy`` files that experiments/lorentz/dataset/generate_dataset.py
writes, it runs the same simulator (``aether_amd.sim``: 'charged' / 'static' / 'dynamic') for the requested seeds in one
launch and leaves everything in HBM.  ``batches(batch_size)`` yields whole batches in the flattened layout the runner
builds per batch (main.py:205-246: ``[B n, 3]`` positions / velocities, ``edge_attr = [q_i q_j, |x_i - x_j|]``, the
edge index of ``get_edges``), so the training loop does no host-side work per batch.
"""
from __future__ import annotations

import torch

from . import sim as _sim
from .edges import get_edges, prepare_edge_attr

_SIMS = {"charged": _sim.ChargedParticlesSim, "static": _sim.GravitySim, "dynamic": _sim.DynamicSim,
         "fixcharge": _sim.FixCharge}


class SimulatedNBodyDataset:
    def __init__(self, seeds, simulation="charged", n_balls=5, length=5000, sample_freq=100, device="cuda",
                 frame_0=30, frame_T=40, initial_vel_norm=0.5):
        if simulation not in _SIMS:
            raise ValueError(f"simulation must be one of {sorted(_SIMS)}")
        self.sim = _SIMS[simulation](noise_var=0.0, n_balls=n_balls, vel_norm=initial_vel_norm, device=device)
        loc, vel, edges, charges = self.sim.sample_trajectories(list(seeds), T=length, sample_freq=sample_freq, as_tensor=True)
        if loc.shape[1] <= frame_T:
            raise ValueError("the trajectories are shorter than frame_T")
        # dataset4newton.py:46-48: [S, T, 3, n] -> [S, T, n, 3], fp32
        self.loc = loc.transpose(2, 3).to(torch.float32).contiguous()
        self.vel = vel.transpose(2, 3).to(torch.float32).contiguous()
        self.charges = charges.to(torch.float32)                              # [S, n, 1]
        n = n_balls
        rows, cols = torch.where(~torch.eye(n, dtype=torch.bool, device=self.loc.device))    # i != j, row-major (:56-61)
        self.edges = [rows, cols]
        self.edge_attr = edges.to(torch.float32)[:, rows, cols].unsqueeze(2)  # q_i q_j per edge, [S, n (n - 1), 1]
        self.frame_0, self.frame_T = frame_0, frame_T
        self.n_nodes = n

    def __len__(self):
        return self.loc.shape[0]

    def get_n_nodes(self):
        return self.n_nodes

    def __getitem__(self, i):
        return self.loc[i, self.frame_0], self.vel[i, self.frame_0], self.edge_attr[i], self.charges[i], self.loc[i, self.frame_T]

    def get_edges(self, batch_size, n_nodes):
        return get_edges(batch_size, n_nodes, device=self.loc.device)

    def batches(self, batch_size, drop_last=True):
        """Batches as the runner flattens them (main.py:205-246): dict with x, vel [B n, 3], charges [B n, 1], edges,
        edge_attr [B n (n - 1), 2] = [q_i q_j, distance], h = |v| [B n, 1] and the target positions."""
        n, S = self.n_nodes, len(self)
        for lo in range(0, S - (batch_size - 1 if drop_last else 0), batch_size):
            hi = min(S, lo + batch_size)
            B = hi - lo
            x = self.loc[lo:hi, self.frame_0].reshape(B * n, 3)
            v = self.vel[lo:hi, self.frame_0].reshape(B * n, 3)
            q = self.charges[lo:hi].reshape(B * n, 1)
            edges = self.get_edges(B, n)
            ea = prepare_edge_attr(x, edges, self.edge_attr[lo:hi].reshape(-1, 1))
            yield {"h": v.norm(dim=-1, keepdim=True), "x": x, "vel": v, "charges": q, "edges": edges, "edge_attr": ea,
                   "target": self.loc[lo:hi, self.frame_T].reshape(B * n, 3)}


class SimulatedFieldDataset:
    """The seq2seq runners' data set (experiments/electrostatic/static_electrostatic_field_data.py:8-117: ``feats``
    [S, T, N, 2D] = positions | velocities of the moving particles, the four normalisation modes, ``unnormalize`` /
    ``torch_unnormalize``, items {'inputs', 'edges', 'charges'}) over trajectories simulated on the device with
    ``aether_amd.sim.ElectrostaticFieldSim`` (a static field: the same field sources for every simulation, as
    ``generate_dataset.py --static_field``) instead of the ``*_feats`` files.  ``stats_from``: another
    ``SimulatedFieldDataset`` (the training split) whose statistics normalise this one, as the reference normalises
    validation / test data with the training set's statistics (:40-62)."""

    def __init__(self, num_sims, params=None, n_balls=5, static_balls=20, ndim=2, length=5000, sample_freq=100, box_size=5.0,
                 particle_seed=0, field_seed=1, device="cuda", stats_from=None):
        params = params or {}
        self.ndim = ndim
        self.same_norm = params.get("same_data_norm", False)
        self.symmetric_norm = params.get("symmetric_data_norm", False)
        self.no_norm = params.get("no_data_norm", False)
        self.vel_norm_norm = params.get("vel_norm_norm", False)
        sim = _sim.ElectrostaticFieldSim(noise_var=0.0, n_balls=n_balls, static_balls=static_balls, box_size=box_size, dim=ndim,
                                         device=device)
        sim._particle_seed, sim._field_seed = particle_seed, field_seed
        sim.reset_particle_rng()
        loc, vel, edges, charges = sim.sample_trajectories(num_sims, T=length, sample_freq=sample_freq,
                                                           reset_field_rng=static_balls > 0, as_tensor=True)
        n = n_balls
        self.feats = torch.cat([loc[:, :, :n], vel[:, :, :n]], -1).to(torch.float32)       # [S, T, N, 2D]
        self.edges = edges[:, :n, :n].to(torch.float32)
        self.charges = charges[:, :n, 0].to(torch.float32)
        self.static_field = loc[0, 0, n:].to(torch.float32)
        self.static_charges = charges[0, n:].to(torch.float32)
        if not self.no_norm:
            self._normalize_data(self.feats if stats_from is None else stats_from._raw)
        self._raw = self.feats if self.no_norm else self._raw

    def _normalize_data(self, train):
        D = self.ndim
        self._raw = self.feats.clone()
        if self.same_norm:
            self.feat_max, self.feat_min = train.max(), train.min()
            self.feats = (self.feats - self.feat_min) * 2 / (self.feat_max - self.feat_min) - 1
        elif self.vel_norm_norm:
            self.vel_norm_max = train[..., D:].norm(dim=-1).max()
            self.feats = self.feats / self.vel_norm_max
        else:
            if self.symmetric_norm:
                self.loc_max, self.vel_max = train[..., :D].abs().max(), train[..., D:].abs().max()
                self.loc_min, self.vel_min = -self.loc_max, -self.vel_max
            else:
                self.loc_max, self.loc_min = train[..., :D].max(), train[..., :D].min()
                self.vel_max, self.vel_min = train[..., D:].max(), train[..., D:].min()
            self.feats = torch.cat([(self.feats[..., :D] - self.loc_min) * 2 / (self.loc_max - self.loc_min) - 1,
                                    (self.feats[..., D:] - self.vel_min) * 2 / (self.vel_max - self.vel_min) - 1], -1)

    def torch_unnormalize(self, data):
        D = self.ndim
        if self.no_norm:
            return data
        if self.same_norm:
            return (data + 1) * (self.feat_max - self.feat_min) / 2. + self.feat_min
        if self.vel_norm_norm:
            return data * self.vel_norm_max
        return torch.cat([(data[..., :D] + 1) * (self.loc_max - self.loc_min) / 2. + self.loc_min,
                          (data[..., D:] + 1) * (self.vel_max - self.vel_min) / 2. + self.vel_min], -1)

    def unnormalize(self, data):
        return self.torch_unnormalize(torch.as_tensor(data, device=self.feats.device)).cpu().numpy()

    def __getitem__(self, idx):
        return {"inputs": self.feats[idx], "edges": self.edges[idx], "charges": self.charges[idx]}

    def __len__(self):
        return len(self.feats)


def burn_in_masks_of(masks, max_burn_in_count):
    """The data set's burn-in masks (experiments/ind/single_ind_data.py:73-81) for masks [..., T, N] of zeros and ones: an
    object is observed at its first ``max_burn_in_count`` present frames.  The reference's loop counts the observed frames
    of an object so far and compares with the limit; that count is min(exclusive cumsum of the mask, limit), so the mask
    is  masks * (exclusive cumsum over time < max_burn_in_count)  -- one cumsum, on whatever device ``masks`` is."""
    m = (masks == 1).to(torch.float32)
    seen = torch.cumsum(m, dim=-2) - m
    return m * (seen < max_burn_in_count).to(torch.float32)


class SceneDataset:
    """The inD runner's data set (experiments/ind/single_ind_data.py ``IndData``) kept on the device, for evaluation:
    padded scenes, burn-in masks, un-normalisation, and batches that carry a ``ScenePack`` (the per-frame graphs of the
    batch, built on the device in one library call) instead of per-scene Python lists.  There is no inD file loader: the
    recordings are licensed.  The caller hands over the normalised tracks.

    ``feats`` / ``masks``: per-scene tensors [T_s, N_s, 4] / [T_s, N_s] or padded ones [S, T, N, 4] / [S, T, N]; scenes
    are zero-padded to the longest and the widest as ``ind_collate_fn`` does (:235-256).  ``stats``: None, a scalar
    ``vel_norm_max`` or ``(min_feats, max_feats)`` -- what the reference loads from its two statistics files (:122-141).
    ``non_linear_masks``: [S][N_s] flags (the reference's attribute of that name); evaluation skips tracks whose flag is 0.
    """

    def __init__(self, feats, masks, max_burn_in_count=-1, stats=None, non_linear_masks=None, k=10, device="cuda"):
        feats = list(feats) if not torch.is_tensor(feats) else list(feats.unbind(0))
        masks = list(masks) if not torch.is_tensor(masks) else list(masks.unbind(0))
        if len(feats) != len(masks) or not feats:
            raise ValueError("SceneDataset: feats and masks must hold the same, non-zero number of scenes")
        self.device, self.k = torch.device(device), int(k)
        self.shapes = [(int(f.shape[0]), int(f.shape[1])) for f in feats]
        S, T, N = len(feats), max(s[0] for s in self.shapes), max(s[1] for s in self.shapes)
        self.feats = torch.zeros(S, T, N, 4, dtype=torch.float32, device=self.device)
        self.masks = torch.zeros(S, T, N, dtype=torch.float32, device=self.device)
        for i, (f, m) in enumerate(zip(feats, masks)):
            if tuple(m.shape) != self.shapes[i] or f.shape[-1] != 4:
                raise ValueError(f"SceneDataset: scene {i}: feats must be [T, N, 4] and masks [T, N]")
            self.feats[i, :f.shape[0], :f.shape[1]] = f.to(self.device, torch.float32)
            self.masks[i, :m.shape[0], :m.shape[1]] = m.to(self.device, torch.float32)
        self.max_burn_in_count = max_burn_in_count
        self.burn_in_masks = burn_in_masks_of(self.masks, max_burn_in_count)
        self.vel_norm_norm = stats is not None and not isinstance(stats, (tuple, list))
        one = torch.ones(4, dtype=torch.float32, device=self.device)
        if stats is None:
            self.scale, self.offset = one, torch.zeros_like(one)
        elif self.vel_norm_norm:
            self.scale = one * torch.as_tensor(stats, dtype=torch.float32, device=self.device).reshape(())
            self.offset = torch.zeros_like(one)
        else:
            lo, hi = (torch.as_tensor(s, dtype=torch.float32, device=self.device).reshape(-1) * one for s in stats)
            self.scale, self.offset = (hi - lo) / 2.0, (hi - lo) / 2.0 + lo           # (x + 1) (max - min) / 2 + min
        self.non_linear_masks = None
        if non_linear_masks is not None:
            self.non_linear_masks = torch.zeros(S, N, dtype=torch.float32, device=self.device)
            for i, nl in enumerate(non_linear_masks):
                nl = torch.as_tensor(nl).to(self.device, torch.float32).reshape(-1)
                self.non_linear_masks[i, :nl.numel()] = nl

    def unnormalize_data(self, feats):
        """:122-141 for a tensor [..., 4]."""
        return feats * self.scale.to(feats.device) + self.offset.to(feats.device)

    def __len__(self):
        return len(self.shapes)

    def __getitem__(self, index):
        """The reference's entry (:177-183) of one scene, un-padded: node_inds[t] and graph_info[t] are views into a
        one-scene pack, in the form ``predict_future`` takes after ``ind_collate_fn`` / ``unsqueeze(0)``."""
        from .nn.dynamicvars.aether_dynamicvars import pack_scenes
        T, N = self.shapes[index]
        sl = (slice(index, index + 1), slice(0, T), slice(0, N))
        node_inds, graph_info = pack_scenes(self.feats[sl], self.masks[sl], self.k).as_lists()
        return {"inputs": self.feats[sl][0], "masks": self.masks[sl][0], "burn_in_masks": self.burn_in_masks[sl][0],
                "node_inds": node_inds[0], "graph_info": graph_info[0]}

    def batches(self, batch_size):
        """Padded batches in data-set order: the tensors of ``ind_collate_fn`` plus ``pack`` (a ``ScenePack`` of the batch)
        and ``keep`` (the batch's non_linear_masks, or None)."""
        from .nn.dynamicvars.aether_dynamicvars import pack_scenes
        for lo in range(0, len(self), batch_size):
            sl = slice(lo, lo + batch_size)
            yield {"inputs": self.feats[sl], "masks": self.masks[sl], "burn_in_masks": self.burn_in_masks[sl],
                   "pack": pack_scenes(self.feats[sl], self.masks[sl], self.k),
                   "keep": None if self.non_linear_masks is None else self.non_linear_masks[sl]}
