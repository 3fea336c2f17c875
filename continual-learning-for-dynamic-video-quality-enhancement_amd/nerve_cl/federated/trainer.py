"""Federated rounds in one process: FedAvg over whole-model weight vectors, optional clipping of the client updates, server
learning rate and Gaussian noise, as one pass of csrc/federated.hip over a matrix whose rows are the clients' weights
(DESIGN.md section 23).

The reference's ``FederatedTrainer.train_round`` (reference nerve_cl/federated/server.py:141-193) selects clients and counts
samples but neither trains nor aggregates; here a round trains every selected client on the model itself (its flat parameter
buffer is reset to the global weights in place, so parameters are never re-homed and captured graphs stay valid) and averages
on the device.  ``flwr`` is only the transport between processes and is not needed for any of this; it is still not implemented.

With ``num_clusters > 1`` the trainer is clustered federated learning: one round clusters the clients by
their updates (csrc/cluster.hip) and from then on every cluster has its own model, stepped by its own clients.
"""
from __future__ import annotations

import random
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from nerve_cl import _engine, _nvq
from nerve_cl._bucket import segments_of
from nerve_cl.federated._flat import check_clients, device_weights, finish_cpu, host_weights
from nerve_cl.federated.compression import COMPRESSIONS, compress_updates_, topk_count
from nerve_cl.federated.fedopt import ServerOptimizer
from nerve_cl.federated.privacy import DPOptimizer, PrivacyConfig, _Seg

__all__ = ["aggregate_flat", "fedavg", "weighted_average", "FederatedTrainer", "start_server", "AGGREGATORS"]

AGGREGATORS = ("fedavg", "median", "trimmed_mean", "krum", "multi_krum")


# ----------------------------------------------------------------------------------------------- aggregation
def aggregate_flat(clients: torch.Tensor, weights, base: Optional[torch.Tensor] = None, clip_norm: Optional[float] = None,
                   server_lr: float = 1.0, noise_std: float = 0.0, seed: int = 0, offset: int = 0,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[i] = base[i] + server_lr * sum_k c_k (clients[k, i] - base[i]) + noise_std * z_i`` for a ``[K, n]`` fp32 matrix of
    client weight vectors (a row stride above n is fine), ``c_k = weights[k] / sum(weights) * min(1, clip_norm / (|x_k - base| +
    1e-6))`` (no ``clip_norm``: no clipping; no ``base``: zeros, so the defaults are plain FedAvg).  ``z`` is the Philox stream
    (seed, offset) of ``nerve_cl.federated._philox``.  ``out`` may be ``base``.

    On the GPU: ``nvq_fed_delta_norms`` (only with ``clip_norm``) and ``nvq_fed_aggregate``, nothing read back; ``weights`` given
    as a float64 tensor on the device is used as it is (all-zero weights then give NaN), otherwise it is checked on the host and
    all-zero weights raise ``ValueError``.  CPU tensors take the same formula in float64 torch operations."""
    check_clients(clients, base)
    K, n = clients.shape
    host = host_weights(weights, K, "aggregate_flat", allow_none=False, need="sum")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=clients.device)
    if clients.is_cuda:
        dev = clients.device
        weights = device_weights(weights, host, dev)
        with _nvq.device_guard(dev):
            sq = None
            if clip_norm is not None:
                sq = torch.empty(K, dtype=torch.float64, device=dev)
                _nvq.fed_delta_norms(clients, n, base, sq, _engine.workspace(dev))
            _nvq.fed_aggregate(clients, n, base, weights, sq, out, clip_norm=clip_norm or 0.0, server_lr=server_lr,
                               noise_std=noise_std, seed=seed, offset=offset)
        return out
    w = torch.as_tensor(host if host is not None else weights, dtype=torch.float64)
    x = clients.double()
    b = base.double().view(1, n) if base is not None else torch.zeros(1, n, dtype=torch.float64)
    d = x - b
    c = w / w.sum()
    if clip_norm is not None:
        c = c * torch.clamp(clip_norm / (d.pow(2).sum(1).sqrt() + 1e-6), max=1.0)
    return finish_cpu(b[0] + server_lr * (c.view(K, 1) * d).sum(0), noise_std, seed, offset, out)


def _is_float(t: torch.Tensor) -> bool:
    return t.is_floating_point()


def _int_mean(stack: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """weighted mean of integer tensors truncated toward zero (what a float average cast back to the integer type gives)"""
    mean = (stack.double() * w.view(-1, *([1] * (stack.dim() - 1)))).sum(0) / w.sum()
    return mean.trunc().to(stack.dtype)


def fedavg(states: "Sequence[Dict[str, torch.Tensor]]", num_examples: Sequence[float]) -> "Dict[str, torch.Tensor]":
    """Sample-weighted average of state dicts (FedAvg, McMahan et al. 2017): floating tensors through ``aggregate_flat`` as one
    packed row per client, integer buffers (``num_batches_tracked``) as the weighted mean truncated toward zero."""
    if len(states) == 0 or len(states) != len(num_examples):
        raise ValueError("fedavg: one example count per state dict, at least one")
    host = [float(w) for w in num_examples]
    if any(w < 0 for w in host) or not sum(host) > 0:
        raise ValueError("fedavg: the example counts are non-negative and not all zero")
    keys = list(states[0].keys())
    fkeys = [k for k in keys if _is_float(states[0][k])]
    out: "Dict[str, torch.Tensor]" = {}
    if fkeys:
        dev = states[0][fkeys[0]].device
        rows = torch.stack([torch.cat([sd[k].detach().reshape(-1).to(device=dev, dtype=torch.float32) for k in fkeys])
                            for sd in states])
        flat = aggregate_flat(rows, host)
        off = 0
        for k in fkeys:
            t = states[0][k]
            out[k] = flat[off:off + t.numel()].view(t.shape).to(t.dtype)
            off += t.numel()
    for k in keys:
        if k not in out:
            stack = torch.stack([sd[k].detach() for sd in states])
            out[k] = _int_mean(stack, torch.tensor(host, dtype=torch.float64).to(stack.device))
    return {k: out[k] for k in keys}


def weighted_average(metrics: "List[Tuple[int, Dict[str, float]]]") -> "Dict[str, float]":
    """[(num_samples, {name: value})] -> {name: the sample-weighted mean} (reference server.py:99-110)"""
    total = sum(n for n, _ in metrics)
    acc: "Dict[str, float]" = {}
    for n, m in metrics:
        for k, v in m.items():
            acc[k] = acc.get(k, 0.0) + n * v
    return {k: v / total for k, v in acc.items()}


def start_server(model: nn.Module, num_rounds: int = 100, server_address: str = "[::]:8080", min_clients: int = 2) -> None:
    """The networked server is flwr's; this package implements the arithmetic of a round, not the transport."""
    try:
        import flwr  # noqa: F401
    except ImportError as e:
        raise ImportError("start_server needs the `flwr` package (the transport between server and clients); without it use "
                          "FederatedTrainer, which runs the same rounds in one process") from e
    raise NotImplementedError("the flwr server strategy is not part of this package; FederatedTrainer runs the rounds in one process")


# ----------------------------------------------------------------------------------------------- the trainer
class _Pack:
    """Tensors of a state dict packed into one fp32 row (each at a multiple of 4 floats)"""

    def __init__(self, tensors: "List[torch.Tensor]"):
        self.tensors = tensors
        self.offsets, off = [], 0
        for t in tensors:
            self.offsets.append(off)
            off += (t.numel() + 3) // 4 * 4
        self.total = off

    def views(self, row: torch.Tensor) -> "List[torch.Tensor]":
        return [row[o:o + t.numel()].view(t.shape) for o, t in zip(self.offsets, self.tensors)]

    def pack(self, row: torch.Tensor) -> None:
        for v, t in zip(self.views(row), self.tensors):
            v.copy_(t)

    def unpack(self, row: torch.Tensor) -> None:
        for v, t in zip(self.views(row), self.tensors):
            t.copy_(v)


class FederatedTrainer:
    """``FederatedTrainer(model, num_clients=10, clients_per_round=5, local_epochs=5, *, lr=1e-4, batch_size=16, loss=None,
    privacy=None, update_clip=None, update_noise=0.0, server_lr=1.0, optimizer_impl="torch", seed=None, aggregator="fedavg",
    trim_ratio=0.1, num_byzantine=0, num_selected=None, after_client=None, server_optimizer=None, server_betas=(0.9, 0.99),
    server_tau=1e-3, prox_mu=0.0, compression=None, compress_ratio=0.01, compress_levels=127, error_feedback=True)``

    ``model(inputs) -> outputs`` is trained on every client's ``(inputs, targets)`` (``set_client_data``) with a fresh
    ``AdamW(lr)`` for ``local_epochs`` passes in batches of ``batch_size``, taken in order; ``loss`` defaults to ``nn.MSELoss()``
    (the reference client's criterion).  ``privacy`` (a ``PrivacyConfig``) wraps the optimizer in ``DPOptimizer``.  ``update_clip``
    clips every client's whole update ``x_k - global`` to that 2-norm, ``update_noise`` is the standard deviation of the Gaussian
    noise added to the aggregated weights, ``server_lr`` scales the aggregated update.  ``optimizer_impl``: ``"torch"`` or ``"bucket"``
    (``nerve_cl.optim.BucketAdamW``).  ``seed`` fixes the client selection and every noise stream; without it the selection is
    ``random.sample`` of the global generator, as in the reference.

    ``num_clusters > 1`` (at most 8, ``num_clients`` at most 64, no ``update_clip``): rounds ``1 .. cluster_after`` are plain FedAvg;
    round ``cluster_after + 1`` trains every client with data from the global model, clusters the rows by their updates
    (``cluster_updates`` on the largest flat buffer; the labels are read to the host once and become ``client_cluster``) and forms
    ``cluster_models``, one ``[C, n]`` device matrix per HIP-backed network, with one ``nvq_fed_aggregate_clusters`` each.  Later
    rounds restore each selected client from its cluster's row, step all cluster models in place with one
    ``nvq_fed_aggregate_clusters`` per network (a cluster with no selected client keeps its model; with ``update_noise`` every
    cluster's row receives its draw) and leave the sample-weighted mean of the cluster models in the model itself.
    There is no re-clustering: a client whose data arrives after the split round belongs to no cluster, and a round that selects it
    raises ``ValueError``.  A selected client without samples is left out of its cluster's step.  ``load_cluster(c)`` copies a cluster's model into the network, ``load_mean()`` the weighted mean again; the round dict gains ``"clusters"``, the sizes.

    ``aggregator``: ``"fedavg"`` (above), or a Byzantine-robust rule on the same client matrix (``nerve_cl.federated.robust``, DESIGN.md
    section 28; no ``update_clip``, no clusters): ``"median"`` and ``"trimmed_mean"`` (per coordinate, ``int(trim_ratio * m)`` values
    dropped from each side, ``m`` the selected clients with samples) are one ``nvq_fed_trimmed_aggregate`` per matrix; ``"krum"`` and
    ``"multi_krum"`` select 1 or ``num_selected`` (default ``m - num_byzantine``) clients by the Gram matrix of their whole updates and
    average those, and the round dict gains ``"selected_weights"`` (1.0 per chosen client, in the order of ``last_selected``).  A
    client without samples is never read by these rules, and integer buffers take the mean over the Krum selection, else the
    sample-weighted one.  ``after_client(client_id, model)`` is called under ``no_grad`` after a client's local training and before
    its weights are copied into its row: the hook with which a script or a test inspects or poisons a client.

    ``server_optimizer`` (``server_betas=(0.9, 0.99)``, ``server_tau=1e-3``): one of ``SERVER_OPTIMIZERS`` (``"fedavgm"``,
    ``"fedadagrad"``, ``"fedadam"``, ``"fedyogi"``: FedOpt, ``nerve_cl.federated.fedopt``; no clusters).  The
    aggregated update is the pseudo-gradient of a server optimizer whose learning rate is ``server_lr``.  BEWARE: an adaptive rule
    moves every coordinate by about ``server_lr`` per round; the default 1.0 is a FedAvg value, not an Adam value (try 1e-3 ..
    1e-1).  Each HIP-backed network's matrix takes ``nvq_fed_server_opt`` in place of ``nvq_fed_aggregate`` (still one launch, two
    with ``update_clip``).  With a robust ``aggregator`` the rule first runs alone into a persistent scratch vector and the ``K =
    1`` form of the kernel steps from the snapshot towards it with the round's noise: the pseudo-gradient is then that of the fp32
    aggregate.  The server optimizer steps parameters only.  BatchNorm statistics and integer buffers always take the plain rule
    (next to HIP-backed networks the rest matrix does so as a whole, its loose parameters included); for a model without
    HIP-backed networks the floating parameters are then packed first and the floating buffers after them, and only the
    parameters' columns take the server step (without ``server_optimizer`` the packing stays in state-dict order).
    ``server_state_dict()`` / ``load_server_state_dict()`` carry the moments.

    ``prox_mu > 0`` is FedProx: after ``loss.backward()`` and before the (DP) optimizer step every trainable parameter's gradient
    gains ``prox_mu * (theta - theta_restored)``, ``theta_restored`` being what the client was reset to (the round snapshot, or its
    cluster's model).  A bucketed network whose gradients are its bucket takes one ``nvq_fed_prox_grad``; loose parameters,
    networks with frozen layers and CPU modules one ``add_`` per parameter.  ``prox_mu = 0`` launches nothing.

    ``compression``: one of ``COMPRESSIONS`` (``nerve_cl.federated.compression``; no clusters).  After the last
    client of a round and before the aggregation, every HIP-backed network's rows take one ``nvq_fed_compress`` against the round
    snapshot: ``"topk"`` keeps the ``topk_count(n, compress_ratio)`` largest coordinates of every client's update, ``"quant"``
    quantises the update to ``compress_levels`` levels of its largest magnitude (QSGD), ``"topk_quant"`` does both.  With
    ``error_feedback`` what a client did not send is kept in its row of a persistent ``[num_clients, n]`` residual matrix per
    network (a client takes the next free row when it is first selected) and added to its next update;
    ``compression_state_dict()`` / ``load_compression_state_dict()`` carry these.  The rules above see only the compressed rows, so
    every one of them works unchanged.  BatchNorm statistics, the rest matrix next to HIP-backed networks and integer buffers are
    never compressed; for a model without HIP-backed networks the floating parameters are packed first (as with
    ``server_optimizer``) and only their columns are.  The Philox seed is the second draw of ``random.Random(seed)``, network j in
    round g (counted from 0) uses the streams ``(g * (len(nets) + 1) + j) * 64 + row``.  The round dict gains ``"kept"``: per
    compressed matrix the kept coordinates of every row (int32 on the device; ``train_round`` gives lists).

    On the GPU the weights of every HIP-backed network inside ``model`` are one flat buffer: the clients' results are the rows of a
    persistent ``[clients_per_round, n]`` matrix and a round ends with one ``nvq_fed_delta_norms`` (only with ``update_clip``) and
    one ``nvq_fed_aggregate`` writing into ``flat_theta()``.  Everything else in the state dict (BatchNorm statistics, loose
    parameters) is packed per client into a second, small matrix and takes the same kernel without clipping, noise or server
    rate; integer buffers take the weighted mean truncated toward zero.  Client data that already lives on the model's device
    is used in place; then nothing is read back between local training and the aggregated weights (``train_round_device``)."""

    def __init__(self, model: nn.Module, num_clients: int = 10, clients_per_round: int = 5, local_epochs: int = 5, *,
                 lr: float = 1e-4, batch_size: int = 16, loss=None, privacy: Optional[PrivacyConfig] = None,
                 update_clip: Optional[float] = None, update_noise: float = 0.0, server_lr: float = 1.0,
                 optimizer_impl: str = "torch", seed: Optional[int] = None, num_clusters: int = 1, cluster_after: int = 0,
                 aggregator: str = "fedavg", trim_ratio: float = 0.1, num_byzantine: int = 0, num_selected: Optional[int] = None,
                 after_client=None, server_optimizer: Optional[str] = None, server_betas: Sequence[float] = (0.9, 0.99),
                 server_tau: float = 1e-3, prox_mu: float = 0.0, compression: Optional[str] = None, compress_ratio: float = 0.01,
                 compress_levels: int = 127, error_feedback: bool = True):
        if not 1 <= num_clusters <= _nvq.CLUSTER_MAX:
            raise ValueError(f"num_clusters: 1 .. {_nvq.CLUSTER_MAX}")
        if server_optimizer is not None:
            ServerOptimizer(server_optimizer, server_lr, server_betas, server_tau)     # its checks: ValueError
            if num_clusters > 1:
                raise NotImplementedError("server_optimizer with num_clusters > 1: there are no per-cluster server moments")
        if not prox_mu >= 0.0:
            raise ValueError(f"invalid prox_mu: {prox_mu}")
        if compression is not None:
            if compression not in COMPRESSIONS:
                raise ValueError(f"compression {compression!r}: one of {', '.join(COMPRESSIONS)}")
            if not 0.0 < compress_ratio <= 1.0:
                raise ValueError(f"invalid compress_ratio: {compress_ratio}")
            if int(compress_levels) != compress_levels or not 1 <= compress_levels <= _nvq.FED_COMPRESS_MAX_LEVELS:
                raise ValueError(f"compress_levels: 1 .. {_nvq.FED_COMPRESS_MAX_LEVELS}, got {compress_levels}")
            if num_clusters > 1:
                raise NotImplementedError("compression with num_clusters > 1: every cluster's clients start from another model, "
                                          "so there is no single base their rows are updates of")
        if cluster_after < 0:
            raise ValueError(f"invalid cluster_after: {cluster_after}")
        if num_clusters > 1 and num_clients > _nvq.FED_MAX_CLIENTS:
            raise ValueError(f"num_clients: at most {_nvq.FED_MAX_CLIENTS} with clusters (the split round takes every client)")
        if num_clusters > 1 and update_clip is not None:
            raise NotImplementedError("update_clip with num_clusters > 1: per-cluster bases have no single update norm")
        if optimizer_impl not in ("torch", "bucket"):
            raise ValueError(f"optimizer_impl {optimizer_impl!r}: 'torch' or 'bucket'")
        if aggregator not in AGGREGATORS:
            raise ValueError(f"aggregator {aggregator!r}: one of {', '.join(AGGREGATORS)}")
        if aggregator != "fedavg" and update_clip is not None:
            raise NotImplementedError("update_clip with a robust aggregator: the clip coefficient is per row and breaks the "
                                      "ordering the rows of a coordinate share")
        if aggregator != "fedavg" and num_clusters > 1:
            raise NotImplementedError("num_clusters > 1 with a robust aggregator")
        if not trim_ratio >= 0.0:
            raise ValueError(f"invalid trim_ratio: {trim_ratio}")
        if num_byzantine < 0:
            raise ValueError(f"invalid num_byzantine: {num_byzantine}")
        if num_selected is not None and num_selected < 1:
            raise ValueError(f"invalid num_selected: {num_selected}")
        if clients_per_round < 1 or clients_per_round > _nvq.FED_MAX_CLIENTS:
            raise ValueError(f"clients_per_round: 1 .. {_nvq.FED_MAX_CLIENTS}")
        if update_clip is not None and not update_clip > 0.0:
            raise ValueError(f"invalid update_clip: {update_clip}")
        if update_noise < 0.0:
            raise ValueError(f"invalid update_noise: {update_noise}")
        self.model = model
        self.num_clients = num_clients
        self.clients_per_round = clients_per_round
        self.local_epochs = local_epochs
        self.lr, self.batch_size = lr, batch_size
        self.loss = loss if loss is not None else nn.MSELoss()
        self.privacy = privacy
        self.update_clip, self.update_noise, self.server_lr = update_clip, float(update_noise), float(server_lr)
        self.optimizer_impl = optimizer_impl
        self.aggregator, self.trim_ratio = aggregator, float(trim_ratio)
        self.num_byzantine, self.num_selected = int(num_byzantine), num_selected
        self.after_client = after_client
        self.server_optimizer, self.prox_mu = server_optimizer, float(prox_mu)
        self.server_betas, self.server_tau = (float(server_betas[0]), float(server_betas[1])), float(server_tau)
        self._server_opts: List[ServerOptimizer] = []         # one per stepped parameter vector, in the order of _aggregate
        self.seed = seed
        self._rng = random.Random(seed) if seed is not None else random
        self._noise_seed = random.Random(seed).getrandbits(62) if seed is not None else random.getrandbits(62)
        self.compression, self.compress_ratio = compression, float(compress_ratio)
        self.compress_levels, self.error_feedback = int(compress_levels), bool(error_feedback)
        self._compress_seed = 0
        if compression is not None:                    # a stream of its own: the second draw, the first is the noise seed
            draws = random.Random(seed) if seed is not None else random
            if seed is not None:
                draws.getrandbits(62)
            self._compress_seed = draws.getrandbits(62)
        self._residuals: Optional[List[torch.Tensor]] = None   # per compressed matrix [num_clients, n], made with the plan
        self._residual_slot: Dict[int, int] = {}              # client id -> its row of the residual matrices
        self.client_data: Dict[int, Tuple] = {}
        self.global_round = 0
        self.last_selected: List[int] = []
        self._plan = None
        self.num_clusters, self.cluster_after = num_clusters, cluster_after
        self.client_cluster: Dict[int, int] = {}              # client id -> cluster, filled by the split round
        self.cluster_models: Optional[List[torch.Tensor]] = None   # per HIP-backed network a [C, n] matrix, after the split round
        self.cluster_result = None                            # the split round's ClusterResult, on the clients' device

    def set_client_data(self, client_id: int, data: Tuple) -> None:
        """``data``: ``(inputs, targets)`` tensors with one sample per row"""
        self.client_data[client_id] = data

    # ------------------------------------------------------------------ what a round moves
    def _build_plan(self):
        model = self.model
        segs = segments_of(model)
        dev = next(model.parameters()).device
        nets = [sg.net for sg in segs if sg.net is not None] if dev.type == "cuda" else []
        flat_names = {n for sg in segs if sg.net is not None and dev.type == "cuda" for n in sg.names}
        sd = model.state_dict()                       # detached tensors that share the parameters' and buffers' memory
        rest_names = [k for k, t in sd.items() if k not in flat_names and _is_float(t)]
        params = dict(model.named_parameters())
        n_params = 0
        if (self.server_optimizer is not None or self.compression is not None) and not nets:
            # the server optimizer steps, and the compression sparsifies, parameters only: they come first
            first = [k for k in rest_names if k in params]
            rest_names = first + [k for k in rest_names if k not in params]
            n_params = _Pack([sd[k] for k in first]).total
        rest_f = [sd[k] for k in rest_names]
        rest_i = [t for k, t in sd.items() if k not in flat_names and not _is_float(t)]
        K = self.clients_per_round if self.num_clusters == 1 else max(self.clients_per_round, self.num_clients)
        plan = {"dev": dev, "nets": nets, "pack": _Pack(rest_f), "ints": rest_i, "n_params": n_params,
                # FedProx: the trainable parameters of the rest matrix with their place in the pack
                "prox_rest": [(params[k], i) for i, k in enumerate(rest_names) if k in params and params[k].requires_grad],
                "rows": [torch.zeros(K, net._bucket_layout()[1], dtype=torch.float32, device=dev) for net in nets],
                "snaps": [torch.zeros(net._bucket_layout()[1], dtype=torch.float32, device=dev) for net in nets],
                "weights": torch.zeros(K, dtype=torch.float64, device=dev),
                "sq": torch.zeros(K, dtype=torch.float64, device=dev),
                "one": torch.ones(1, dtype=torch.float64, device=dev), "scratch": {},
                "dp_segs": [_Seg(sg) for sg in segs] if self.privacy is not None else None}
        p = plan["pack"]
        plan["rest_rows"] = torch.zeros(K, max(p.total, 4), dtype=torch.float32, device=dev)
        plan["rest_snap"] = torch.zeros(max(p.total, 4), dtype=torch.float32, device=dev)
        plan["int_rows"] = [torch.zeros((K,) + tuple(t.shape), dtype=t.dtype, device=t.device) for t in rest_i]
        plan["int_snap"] = [torch.zeros_like(t) for t in rest_i]
        if self.compression is not None and self.error_feedback and self._residuals is None:
            sizes = [r.shape[1] for r in plan["rows"]] if nets else ([n_params] if n_params else [])
            self._residuals = [torch.zeros(self.num_clients, n, dtype=torch.float32, device=dev) for n in sizes]
        return plan

    def _make_optimizer(self):
        params = [p for p in self.model.parameters() if p.requires_grad]
        if self.optimizer_impl == "bucket":
            from nerve_cl import optim
            return optim.BucketAdamW(params, lr=self.lr)
        fused = bool(params) and all(p.is_cuda and p.dtype == torch.float32 for p in params)
        return torch.optim.AdamW(params, lr=self.lr, **({"fused": True} if fused else {}))

    def _restore(self, plan) -> None:
        for net, snap in zip(plan["nets"], plan["snaps"]):
            net.flat_theta().copy_(snap)
        plan["pack"].unpack(plan["rest_snap"])
        for t, s in zip(plan["ints"], plan["int_snap"]):
            t.copy_(s)

    @torch.no_grad()
    def _prox(self, plan, anchor) -> None:
        """FedProx: every trainable parameter's gradient gains ``prox_mu * (theta - anchor)``.  ``anchor``: (one flat vector per
        HIP-backed network, the packed rest row), what the client was reset to.  A network whose gradients are the views of its
        last gradient bucket takes one ``nvq_fed_prox_grad`` on the bucket; everything else one ``add_`` per parameter."""
        mu = self.prox_mu
        net_anchors, rest_anchor = anchor
        for net, a in zip(plan["nets"], net_anchors):
            mask = net.grad_alias_mask()
            if mask is not None and all(mask):
                with _nvq.device_guard(plan["dev"]):
                    _nvq.fed_prox_grad(net._last_grad_bucket, net.flat_theta(), a, mu)
                continue
            views = net._bucket_views(a)
            for n, p in net._named_params():
                if p.grad is not None:
                    p.grad.add_(p.detach() - views[n], alpha=mu)
        views = plan["pack"].views(rest_anchor)
        for p, i in plan["prox_rest"]:
            if p.grad is not None:
                p.grad.add_(p.detach() - views[i], alpha=mu)

    def _train_client(self, plan, data, seed: int, anchor=None) -> torch.Tensor:
        """local training on the model in place; returns the sum of batch loss x batch size as a 0-dim tensor on the device.
        ``anchor``: what ``_prox`` pulls towards (only read with ``prox_mu > 0``)."""
        dev = plan["dev"]
        xs, ys = data[0], data[1]
        if xs.device != dev:
            xs, ys = xs.to(dev), ys.to(dev)
        opt = self._make_optimizer()
        dp = None
        if self.privacy is not None:
            dp = DPOptimizer(opt, self.model, self.privacy, self.batch_size, max(len(xs), 1), seed=seed, _segments=plan["dp_segs"])
        stepper = dp if dp is not None else opt
        self.model.train()
        total = torch.zeros((), dtype=torch.float32, device=dev)
        for _ in range(self.local_epochs):
            for i in range(0, len(xs), self.batch_size):
                x, y = xs[i:i + self.batch_size], ys[i:i + self.batch_size]
                stepper.zero_grad()
                loss = self.loss(self.model(x), y)
                loss.backward()
                if self.prox_mu > 0.0:
                    self._prox(plan, anchor)
                stepper.step()
                total += loss.detach().float() * len(x)
        return total

    # ------------------------------------------------------------------ a round
    @torch.no_grad()
    def _aggregate(self, plan, K: int, w: torch.Tensor, step) -> None:
        """The walk every rule shares: each HIP-backed network's rows into its flat buffer (network j's noise stream in a round is
        ``global_round * (len(nets) + 1) + j``), the rest matrix into the packed statistics and loose parameters, the integer buffers'
        mean under ``w``.  ``step(rows, n, base, out, *, full, offset)`` aggregates one matrix; ``full``: with the update clip, server
        rate and noise, else the rule alone; ``opt``: the ``ServerOptimizer`` of that vector, which then takes the server step.
        With ``server_optimizer`` the server step is for parameters: the flat buffers, or without a HIP-backed network the
        columns ``[0, n_params)`` of the rest matrix; statistics take the rule alone."""
        nets, pack = plan["nets"], plan["pack"]
        sopt = self.server_optimizer is not None
        plain = self.update_clip is None and self.update_noise == 0.0 and self.server_lr == 1.0 and not sopt
        for j, (net, rows, snap) in enumerate(zip(nets, plan["rows"], plan["snaps"])):
            flat = net.flat_theta()
            step(rows[:K], flat.numel(), None if plain else snap, flat, full=True, offset=self.global_round * (len(nets) + 1) + j,
                 opt=self._server_opt(j) if sopt else None)
        if pack.total:
            rest, snap = plan["rest_rows"][:K], plan["rest_snap"]
            if nets:                                   # next to the flat buffers: statistics and loose parameters, the rule alone
                step(rest, rest.shape[1], None, snap, full=False, offset=0)
            elif sopt:                                 # a plain module: parameters first, then the statistics (_build_plan)
                n_p, total = plan["n_params"], rest.shape[1]
                if n_p:
                    step(rest[:, :n_p], n_p, snap[:n_p], snap[:n_p], full=True, offset=self.global_round, opt=self._server_opt(0))
                if n_p < total:
                    step(rest[:, n_p:], total - n_p, None, snap[n_p:], full=False, offset=0)
            else:                                      # no HIP-backed network (a plain module, any device): everything is here
                step(rest, rest.shape[1], None if plain else snap, snap, full=True, offset=self.global_round)
            pack.unpack(snap)
        for t, rows in zip(plan["ints"], plan["int_rows"]):
            t.copy_(_int_mean(rows[:K], w.to(rows.device)))

    def _server_opt(self, j: int) -> ServerOptimizer:
        """the server optimizer of stepped vector j (a HIP-backed network's flat buffer, or the packed parameters), made on first use"""
        while len(self._server_opts) <= j:
            self._server_opts.append(ServerOptimizer(self.server_optimizer, self.server_lr, self.server_betas, self.server_tau))
        return self._server_opts[j]

    @staticmethod
    def _scratch(plan, n: int) -> torch.Tensor:
        """a persistent fp32 vector of n floats on the plan's device (a robust rule's aggregate before the server step)"""
        if n not in plan["scratch"]:
            plan["scratch"][n] = torch.empty(n, dtype=torch.float32, device=plan["dev"])
        return plan["scratch"][n]

    def server_state_dict(self) -> Dict[str, object]:
        """the server optimizer's state: its name and one ``ServerOptimizer.state_dict()`` per stepped vector (none before the first
        round with ``server_optimizer``)"""
        return {"server_optimizer": self.server_optimizer, "states": [o.state_dict() for o in self._server_opts]}

    def load_server_state_dict(self, state: Dict[str, object]) -> None:
        if state["server_optimizer"] != self.server_optimizer:
            raise ValueError(f"the state is {state['server_optimizer']!r}'s, this trainer runs {self.server_optimizer!r}")
        opts = []
        for sd in state["states"]:
            opt = ServerOptimizer(self.server_optimizer, self.server_lr, self.server_betas, self.server_tau)
            opt.load_state_dict(sd)
            opts.append(opt)
        self._server_opts = opts

    def _step_options(self, full: bool, offset: int) -> Dict[str, object]:
        """the server rate and the noise stream of a ``full`` step as keywords; none for the rule alone"""
        return dict(server_lr=self.server_lr, noise_std=self.update_noise, seed=self._noise_seed, offset=offset) if full else {}

    def _aggregate_fedavg(self, plan, K: int) -> None:
        """FedAvg: per matrix one ``nvq_fed_delta_norms`` (only with ``update_clip``) and one ``nvq_fed_aggregate``"""
        w, clip, dev = plan["weights"][:K], self.update_clip, plan["dev"]

        def step(rows, n, base, out, *, full, offset, opt=None):
            kw = self._step_options(full, offset)
            if opt is not None:                        # FedOpt: nvq_fed_server_opt in place of nvq_fed_aggregate
                kw.pop("server_lr")
                opt.step(rows, w if w.is_cuda else w.tolist(), base, clip_norm=clip, out=out, **kw)
                return
            if not plan["nets"]:                       # the public function: the CPU formula, or the same two launches
                aggregate_flat(rows, w if w.is_cuda else w.tolist(), base=None if base is None else base.clone(), clip_norm=clip,
                               out=out, **kw)
                return
            with _nvq.device_guard(dev):
                sq = None
                if full and clip is not None:
                    sq = plan["sq"]
                    _nvq.fed_delta_norms(rows, n, base, sq, _engine.workspace(dev))
                    kw["clip_norm"] = clip
                _nvq.fed_aggregate(rows, n, base, w, sq, out, **kw)

        self._aggregate(plan, K, w, step)

    # ------------------------------------------------------------------ compressed updates
    @torch.no_grad()
    def _compress(self, plan, selected: List[int], K: int) -> List[torch.Tensor]:
        """Every HIP-backed network's rows, or without one the parameter columns of the rest matrix, take one ``compress_updates_``
        against the round snapshot; returns the kept counts per matrix."""
        nets, mode = plan["nets"], self.compression
        if nets:
            mats = [(rows[:K], snap) for rows, snap in zip(plan["rows"], plan["snaps"])]
        else:
            n_p = plan["n_params"]
            mats = [(plan["rest_rows"][:K, :n_p], plan["rest_snap"][:n_p])] if n_p else []
        slots = None
        if self.error_feedback and mats:
            for cid in selected:
                if cid not in self._residual_slot:
                    if len(self._residual_slot) >= self.num_clients:
                        raise ValueError(f"client {cid} is client number {len(self._residual_slot) + 1}, but num_clients = "
                                         f"{self.num_clients}: the residual matrices have one row per client")
                    self._residual_slot[cid] = len(self._residual_slot)
            slots = [self._residual_slot[cid] for cid in selected]
        kept = []
        for j, (rows, snap) in enumerate(mats):
            n = rows.shape[1]
            kept.append(compress_updates_(rows, snap, k=topk_count(n, self.compress_ratio) if mode.startswith("topk") else None,
                                          levels=self.compress_levels if mode.endswith("quant") else 0,
                                          residual=self._residuals[j] if slots is not None else None, slots=slots,
                                          seed=self._compress_seed, offset=(self.global_round * (len(nets) + 1) + j) * 64))
        return kept

    def compression_state_dict(self) -> Dict[str, object]:
        """the error-feedback state: the mode, every client's row and one residual matrix per compressed matrix (none before the
        first round, or without ``error_feedback``)"""
        return {"compression": self.compression, "slots": dict(self._residual_slot),
                "residuals": [r.clone() for r in self._residuals or []]}

    def load_compression_state_dict(self, state: Dict[str, object]) -> None:
        if state["compression"] != self.compression:
            raise ValueError(f"the state is {state['compression']!r}'s, this trainer runs {self.compression!r}")
        if self._plan is None:
            self._plan = self._build_plan()
        mine = self._residuals or []
        theirs = state["residuals"] or [torch.zeros_like(b) for b in mine]      # saved before the first round: still zero
        if len(theirs) != len(mine) or any(a.shape != b.shape for a, b in zip(theirs, mine)):
            raise ValueError("the residual matrices of the state do not fit this trainer's model and num_clients")
        for a, b in zip(theirs, mine):
            b.copy_(a)
        self._residual_slot = {int(c): int(s) for c, s in state["slots"].items()}

    # ------------------------------------------------------------------ robust rounds
    def _robust_plan(self, counts: List[int]) -> Tuple[int, int]:
        """(trim, number selected) of this round from the sample counts, which the host knows; raises before any client trains"""
        m = sum(1 for c in counts if c > 0)
        f = self.num_byzantine
        if self.aggregator == "median":
            return _nvq.FED_TRIM_MEDIAN, 0
        if self.aggregator == "trimmed_mean":
            trim = int(self.trim_ratio * m + 1e-9)
            if not 2 * trim < m:
                raise ValueError(f"trim_ratio {self.trim_ratio} trims {trim} of {m} clients with samples from each side: nothing is left")
            return trim, 0
        if m < f + 3:
            raise ValueError(f"{self.aggregator}: {m} clients with samples and num_byzantine = {f}: Krum needs at least f + 3")
        if self.aggregator == "krum":
            return 0, 1
        return 0, (self.num_selected if self.num_selected is not None else m - f)

    @torch.no_grad()
    def _aggregate_robust(self, plan, K: int, trim: int, q: int) -> Optional[torch.Tensor]:
        """``_aggregate`` with the robust rules: the sample counts only say which rows are live.  Median and
        trimmed mean: one ``nvq_fed_trimmed_aggregate`` per matrix.  Krum: the Gram of the whole updates (the flat networks' and the
        rest matrix's added), one ``nvq_fed_krum_select``, then the trim-0 pass per matrix with the selection as weights; returns
        the selection."""
        from nerve_cl.federated.clustering import update_gram
        from nerve_cl.federated.robust import aggregate_flat_trimmed, krum_select
        w, pack, selected = plan["weights"][:K], plan["pack"], None
        if q:
            gram = None
            for rows, snap in zip(plan["rows"], plan["snaps"]):
                g = update_gram(rows[:K], snap)
                gram = g if gram is None else gram.add_(g)
            if pack.total:
                g = update_gram(plan["rest_rows"][:K], plan["rest_snap"])
                gram = g if gram is None else gram.add_(g)
            if gram is None:                           # a model without floating state: nothing to tell the clients apart by
                gram = torch.zeros(K, K, dtype=torch.float64, device=w.device)
            w = selected = krum_select(gram, self.num_byzantine, q, weights=w).weights

        def step(rows, n, base, out, *, full, offset, opt=None):   # on the device one nvq_fed_trimmed_aggregate, nothing read back
            if opt is not None:                        # FedOpt: the rule alone into a scratch vector, then the K = 1 server step
                agg = self._scratch(plan, n)
                aggregate_flat_trimmed(rows, trim, weights=w, base=base, out=agg)
                kw = self._step_options(full, offset)
                kw.pop("server_lr")
                one = plan["one"]
                opt.step(agg.view(1, n), one if one.is_cuda else [1.0], base, out=out, **kw)
                return
            aggregate_flat_trimmed(rows, trim, weights=w, base=base, out=out, **self._step_options(full, offset))

        self._aggregate(plan, K, w, step)
        return selected

    # ------------------------------------------------------------------ clustered rounds
    def _cluster_weights(self) -> List[float]:
        """the samples of the clients assigned to each cluster"""
        w = [0.0] * self.num_clusters
        for cid, c in self.client_cluster.items():
            if cid in self.client_data:
                w[c] += float(len(self.client_data[cid][0]))
        return w

    @torch.no_grad()
    def _aggregate_clusters(self, plan, selected: List[int], counts: List[int], K: int, split: bool) -> None:
        """the split round (``split``): cluster the K rows and form the cluster models from the global model; later rounds: step the
        cluster models in place.  Then the model itself receives the sample-weighted mean of the cluster models."""
        from nerve_cl.federated.clustering import aggregate_flat_clustered, cluster_updates
        C, dev, w = self.num_clusters, plan["dev"], plan["weights"][:K]
        nets, pack = plan["nets"], plan["pack"]
        if split:
            if K < C:
                raise ValueError(f"the split round needs at least num_clusters = {C} clients with data, got {K}")
            sizes = [net.flat_theta().numel() for net in nets]
            big = max(range(len(nets)), key=lambda j: sizes[j]) if nets else -1
            if big >= 0 and sizes[big] >= pack.total:
                res = cluster_updates(plan["rows"][big][:K], C, base=plan["snaps"][big])
            else:
                res = cluster_updates(plan["rest_rows"][:K], C, base=plan["rest_snap"])
            self.cluster_result = res
            host = [int(v) for v in res.labels.tolist()]                # the one read-back of clustered training
            self.client_cluster = dict(zip(selected, host))
            self.cluster_models = [torch.zeros(C, n, dtype=torch.float32, device=dev) for n in sizes]
            plan["rest_clusters"] = torch.zeros(C, plan["rest_rows"].shape[1], dtype=torch.float32, device=dev)
            plan["int_clusters"] = [torch.zeros((C,) + tuple(t.shape), dtype=t.dtype, device=t.device) for t in plan["ints"]]
            for ic, snap in zip(plan["int_clusters"], plan["int_snap"]):
                ic.copy_(snap.expand_as(ic))
            plan["labels"] = torch.zeros(plan["weights"].numel(), dtype=torch.int32, device=dev)
            plan["cluster_w"] = torch.zeros(C, dtype=torch.float64, device=dev)
        else:
            host = [self.client_cluster[cid] for cid in selected]
        # A client without samples has weight 0 and label -1 here: it belongs to no cluster in this pass, so a cluster whose
        # selected members all lack samples is an empty cluster and keeps its row instead of dividing by W_c = 0.  The labels
        # are written from the host like the sample counts: no copy, nothing read back.
        labels = plan["labels"][:K]
        for k, c in enumerate(host):
            labels[k].fill_(c if counts[k] > 0 else -1)
        base_off = (self.global_round * (len(nets) + 1)) * C
        for j, (rows, snap, cm) in enumerate(zip(plan["rows"], plan["snaps"], self.cluster_models)):
            aggregate_flat_clustered(rows[:K], w, labels, C, bases=snap if split else cm, server_lr=self.server_lr,
                                     noise_std=self.update_noise, seed=self._noise_seed, offset=base_off + j * C, out=cm)
        if pack.total:
            rc = plan["rest_clusters"]
            if nets:                                   # statistics and loose parameters: a plain step, as in _aggregate
                aggregate_flat_clustered(plan["rest_rows"][:K], w, labels, C, bases=plan["rest_snap"] if split else rc, out=rc)
            else:
                aggregate_flat_clustered(plan["rest_rows"][:K], w, labels, C, bases=plan["rest_snap"] if split else rc,
                                         server_lr=self.server_lr, noise_std=self.update_noise, seed=self._noise_seed,
                                         offset=base_off, out=rc)
        for rows, ic in zip(plan["int_rows"], plan["int_clusters"]):
            for c in range(C):                         # members with samples (known on the host): their weighted mean, by a mask
                if sum(counts[k] for k in range(K) if host[k] == c) > 0:
                    ic[c].copy_(_int_mean(rows[:K], (w * (labels == c)).to(rows.device)))
        self.load_mean()                               # the model: the mean of the cluster models, weighted by their clients' samples

    @torch.no_grad()
    def load_cluster(self, c: int) -> None:
        """copy cluster c's model into the network (for evaluation; the next round restores what it needs itself)"""
        if self.cluster_models is None:
            raise RuntimeError("load_cluster: the split round has not run yet")
        if not 0 <= c < self.num_clusters:
            raise ValueError(f"cluster {c} outside 0 .. {self.num_clusters - 1}")
        plan = self._plan
        for net, cm in zip(plan["nets"], self.cluster_models):
            net.flat_theta().copy_(cm[c])
        plan["pack"].unpack(plan["rest_clusters"][c])
        for t, ic in zip(plan["ints"], plan["int_clusters"]):
            t.copy_(ic[c])

    @torch.no_grad()
    def load_mean(self) -> None:
        """put the sample-weighted mean of the cluster models back into the network (what a round leaves there)"""
        if self.cluster_models is None:
            raise RuntimeError("load_mean: the split round has not run yet")
        plan, dev = self._plan, self._plan["dev"]
        cw_host, cw = self._cluster_weights(), plan["cluster_w"]
        for c, v in enumerate(cw_host):
            cw[c].fill_(v)
        for net, cm in zip(plan["nets"], self.cluster_models):
            with _nvq.device_guard(dev):
                _nvq.fed_aggregate(cm, cm.shape[1], None, cw, None, net.flat_theta())
        if plan["pack"].total:
            aggregate_flat(plan["rest_clusters"], cw if cw.is_cuda else cw_host, out=plan["rest_snap"])
            plan["pack"].unpack(plan["rest_snap"])
        for t, ic in zip(plan["ints"], plan["int_clusters"]):
            t.copy_(_int_mean(ic, cw.to(ic.device)))

    def cluster_sizes(self) -> List[int]:
        """the number of clients assigned to each cluster (zeros before the split round)"""
        sizes = [0] * self.num_clusters
        for c in self.client_cluster.values():
            sizes[c] += 1
        return sizes

    def train_round_device(self) -> Dict[str, object]:
        """One round; ``train_loss`` stays a 0-dim tensor on the device, so with client data on the device nothing is read back
        (the split round of a clustered trainer reads the labels once)."""
        available = list(self.client_data.keys())
        clustered = self.num_clusters > 1 and self.global_round >= self.cluster_after
        split = clustered and self.cluster_models is None
        if split:                                      # every client with data, starting from the global model
            selected = sorted(available)
        else:
            selected = self._rng.sample(available, min(self.clients_per_round, len(available)))
        late = [c for c in selected if c not in self.client_cluster] if clustered and not split else []
        if late:
            raise ValueError(f"clients {late} received data after the split round and belong to no cluster: there is no re-clustering")
        counts = [len(self.client_data[c][0]) for c in selected]
        if selected and not sum(counts) > 0:
            raise ValueError("train_round: every selected client has no samples (all-zero aggregation weights)")
        robust = self._robust_plan(counts) if selected and self.aggregator != "fedavg" else None
        if self._plan is None:
            self._plan = self._build_plan()
        plan = self._plan
        K = len(selected)
        if K > plan["weights"].numel():
            raise ValueError(f"{K} clients with data, but num_clients = {self.num_clients}: the split round takes every client")
        seeds = [self._rng.getrandbits(62) for _ in selected] if self.seed is not None else [random.getrandbits(62) for _ in selected]
        loss_sum = torch.zeros((), dtype=torch.float32, device=plan["dev"])
        with torch.no_grad():
            for net, snap in zip(plan["nets"], plan["snaps"]):
                snap.copy_(net.flat_theta())
            plan["pack"].pack(plan["rest_snap"])
            for t, s in zip(plan["ints"], plan["int_snap"]):
                s.copy_(t)
        for k, (cid, cnt) in enumerate(zip(selected, counts)):
            with torch.no_grad():
                if clustered and not split:
                    c = self.client_cluster[cid]
                    self.load_cluster(c)
                    anchor = ([cm[c] for cm in self.cluster_models], plan["rest_clusters"][c])
                else:
                    self._restore(plan)
                    anchor = (plan["snaps"], plan["rest_snap"])
            loss_sum += self._train_client(plan, self.client_data[cid], seeds[k], anchor)
            with torch.no_grad():
                if self.after_client is not None:
                    self.after_client(cid, self.model)
                for net, rows in zip(plan["nets"], plan["rows"]):
                    rows[k].copy_(net.flat_theta())
                plan["pack"].pack(plan["rest_rows"][k])
                for t, rows in zip(plan["ints"], plan["int_rows"]):
                    rows[k].copy_(t)
                plan["weights"][k].fill_(float(cnt))
        selection = None
        kept = self._compress(plan, selected, K) if K and self.compression is not None else None
        if K and clustered:
            self._aggregate_clusters(plan, selected, counts, K, split)
        elif K and robust is not None:
            selection = self._aggregate_robust(plan, K, *robust)
        elif K:
            self._aggregate_fedavg(plan, K)
        self.global_round += 1
        self.last_selected = selected
        steps = max(sum(counts) * self.local_epochs, 1)
        out = {"round": self.global_round, "clients": K, "samples": sum(counts), "train_loss": loss_sum / steps}
        if self.num_clusters > 1:
            out["clusters"] = self.cluster_sizes()
        if selection is not None:
            out["selected_weights"] = selection
        if kept is not None:
            out["kept"] = kept
        return out

    def train_round(self) -> Dict[str, float]:
        """Execute one federated round: ``{"round", "clients", "samples"}`` as in the reference, plus ``train_loss``, the mean
        training loss per sample over the clients' local steps."""
        out = self.train_round_device()
        out["train_loss"] = float(out["train_loss"])
        if "selected_weights" in out:
            out["selected_weights"] = out["selected_weights"].tolist()
        if "kept" in out:
            out["kept"] = [t.tolist() for t in out["kept"]]
        return out
