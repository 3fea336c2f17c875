"""User clustering for personalised federated learning: the reference's ``UserProfile`` / ``UserClustering`` (reference
nerve_cl/federated/clustering.py) and clustering by model update on the client matrix (csrc/cluster.hip).

Clustering by update works on the ``[K, n]`` matrix whose rows are the clients' weights: ``update_gram`` is the Gram matrix of
the updates ``x_k - base`` in float64 (one pass over the matrix), ``update_similarity`` its cosine form (the quantity of Sattler
et al., "Clustered Federated Learning", 2019), ``cluster_updates`` Lloyd's algorithm in the update space computed from the Gram
alone, and ``aggregate_flat_clustered`` one FedAvg step per cluster in a single pass.  On CUDA tensors these are HIP kernels and
nothing is read back; CPU tensors take the same formulas in float64 numpy / torch operations.

Deliberate differences from the reference:

- Profile clustering does not use scikit-learn.  ``update_clusters`` runs a numpy float64 Lloyd's algorithm with a seeded
  k-means++ start (``UserClustering.RESTARTS`` starts from the seeds 42, 43, ..., the lowest inertia kept).  It is not bit-compatible with ``sklearn.cluster.KMeans(random_state=42)``: the draws
  differ, sklearn tries several candidates per seed and re-seeds empty clusters; on well-separated data both give the same
  partition up to a relabelling.  ``clusterer`` is a small object with ``predict``, ``labels_`` and ``cluster_centers_``.
- Lloyd's rules here, on the host and on the device alike: the centroid of a cluster is the unweighted mean of its members, a
  row goes to the nearest centroid with ties to the lowest cluster index, a cluster that loses all its members stays empty (no
  re-seeding), and the sweeps stop when no label changes or after ``max_iter``.
- ``UserProfile.update_vector`` is not read by ``update_clusters`` (the reference never reads it either);
  ``UserClustering.cluster_updates`` clusters by update from the client matrix itself.
"""
from __future__ import annotations

from collections import Counter
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from nerve_cl import _engine, _nvq
from nerve_cl.federated._flat import check_clients, device_weights, finish_cpu

__all__ = ["UserProfile", "UserClustering", "ClusterResult", "update_gram", "update_similarity", "cluster_updates",
           "aggregate_flat_clustered"]


# ----------------------------------------------------------------------------------------------- Lloyd's algorithm on the host
def _sqdist(X: np.ndarray, centers: np.ndarray, live: np.ndarray) -> np.ndarray:
    d = ((X[:, None, :] - centers[None, :, :]) ** 2).sum(-1)
    d[:, ~live] = np.inf
    return d


def _kmeans_pp(X: np.ndarray, C: int, seed: int) -> np.ndarray:
    """seeded k-means++ (Arthur & Vassilvitskii 2007): row indices of the C seeds"""
    rng = np.random.RandomState(seed)
    idx = [int(rng.randint(len(X)))]
    d = ((X - X[idx[0]]) ** 2).sum(-1)
    for _ in range(1, C):
        total = d.sum()
        nxt = int(np.searchsorted(np.cumsum(d), rng.random_sample() * total, side="right")) if total > 0 else int(rng.randint(len(X)))
        idx.append(min(nxt, len(X) - 1))
        d = np.minimum(d, ((X - X[idx[-1]]) ** 2).sum(-1))
    return np.array(idx)


def _farthest_first(G: np.ndarray, C: int) -> np.ndarray:
    """the device's seeding: the row with the largest G_kk, then the row farthest from the seeds so far; ties to the lowest index"""
    diag = np.diag(G)
    seeds = [int(np.argmax(diag))]
    mind = np.full(len(G), np.inf)
    for _ in range(1, C):
        s = seeds[-1]
        mind = np.minimum(mind, diag - 2.0 * G[:, s] + G[s, s])
        seeds.append(int(np.argmax(mind)))
    return np.array(seeds)


def _lloyd(X: np.ndarray, C: int, init: Optional[Sequence[int]] = None, seed: int = 42, max_iter: int = 300):
    """numpy float64 Lloyd's algorithm on the rows of X: ``(labels, counts, inertia, n_iter, centers)``.  ``init``: C row indices,
    or None for the seeded k-means++ start."""
    X = np.asarray(X, dtype=np.float64)
    seeds = np.asarray(init if init is not None else _kmeans_pp(X, C, seed), dtype=np.int64)
    centers = X[seeds].copy()
    live = np.ones(C, dtype=bool)
    labels = _sqdist(X, centers, live).argmin(1)
    n_iter = 0

    def stats(labels):
        counts = np.bincount(labels, minlength=C)
        centers = np.zeros((C, X.shape[1]))
        for c in range(C):
            if counts[c]:
                centers[c] = X[labels == c].mean(0)
        return counts, centers

    while n_iter < max_iter:
        counts, centers = stats(labels)
        new = _sqdist(X, centers, counts > 0).argmin(1)
        n_iter += 1
        changed = bool((new != labels).any())
        labels = new
        if not changed:
            break
    counts, centers = stats(labels)
    inertia = float(((X - centers[labels]) ** 2).sum())
    return labels.astype(np.int32), counts.astype(np.int32), inertia, n_iter, centers


class _HostKMeans:
    """what ``UserClustering.clusterer`` holds after a fit"""

    def __init__(self, labels: np.ndarray, centers: np.ndarray, counts: np.ndarray):
        self.labels_, self.cluster_centers_, self._live = labels, centers, counts > 0

    def predict(self, features) -> np.ndarray:
        X = np.asarray(features, dtype=np.float64).reshape(-1, self.cluster_centers_.shape[1])
        return _sqdist(X, self.cluster_centers_, self._live).argmin(1)


# ----------------------------------------------------------------------------------------------- clustering by update
class ClusterResult(NamedTuple):
    """``labels`` int32 [K], ``counts`` int32 [C], ``inertia`` float64 scalar, ``n_iter`` int32 scalar, ``gram`` float64 [K, K]:
    tensors on the clients' device"""
    labels: torch.Tensor
    counts: torch.Tensor
    inertia: torch.Tensor
    n_iter: torch.Tensor
    gram: torch.Tensor


_gram_ws: Dict = {}


def _gram_workspace(dev, K: int, n: int) -> torch.Tensor:
    need = _nvq.fed_gram_workspace_bytes(K, n)
    ws = _engine.workspace(dev)
    if ws.numel() * 4 >= need:
        return ws
    ws = _gram_ws.get(dev)
    if ws is None or ws.numel() * 4 < need:
        ws = _gram_ws[dev] = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
    return ws


def update_gram(clients: torch.Tensor, base: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``G[i, j] = sum_t (clients[i, t] - base[t]) (clients[j, t] - base[t])`` as a ``(K, K)`` float64 tensor on the clients' device
    (``base`` None: zeros).  On the GPU one ``nvq_fed_update_gram`` (fp64 matrix cores, symmetric bit for bit), nothing read back."""
    check_clients(clients, base)
    K, n = clients.shape
    if clients.is_cuda:
        dev = clients.device
        gram = torch.empty(K, K, dtype=torch.float64, device=dev)
        with _nvq.device_guard(dev):
            _nvq.fed_update_gram(clients, n, base, gram, _gram_workspace(dev, K, n))
        return gram
    u = clients.double() - (base.double().view(1, n) if base is not None else 0.0)
    return u @ u.t()


def update_similarity(clients: torch.Tensor, base: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The cosine matrix ``G_ij / sqrt(G_ii G_jj)`` of the updates (float64, on the clients' device); a zero update gives 0."""
    g = update_gram(clients, base)
    norm = g.diagonal().clamp_min(0.0).sqrt()
    denom = norm.view(-1, 1) * norm.view(1, -1)
    return torch.where(denom > 0, g / torch.where(denom > 0, denom, torch.ones_like(denom)), torch.zeros_like(g))


def cluster_updates(clients: torch.Tensor, num_clusters: int, base: Optional[torch.Tensor] = None, init=None,
                    max_iter: int = 50) -> ClusterResult:
    """Lloyd's algorithm on the updates ``clients[k] - base`` (``ClusterResult``).  ``init``: ``num_clusters`` distinct row indices (a
    sequence or an int32 tensor) or None: farthest-first seeding (the row with the largest norm, then the row farthest from the
    seeds so far, ties to the lowest index).

    On the GPU three launches (the Gram pass, its finishing launch, ``nvq_cluster_gram_kmeans``) and no synchronisation: every
    field of the result is a device tensor.  CPU tensors take the float64 Lloyd's of this module on the explicit updates."""
    check_clients(clients, base)
    K, n = clients.shape
    C = int(num_clusters)
    if not 1 <= C <= min(_nvq.CLUSTER_MAX, K):
        raise ValueError(f"num_clusters: 1 .. min({_nvq.CLUSTER_MAX}, K = {K})")
    if max_iter < 0:
        raise ValueError("max_iter >= 0")
    if init is not None and not isinstance(init, torch.Tensor):
        host = [int(i) for i in init]
        if len(host) != C or len(set(host)) != C or any(not 0 <= i < K for i in host):
            raise ValueError("init: num_clusters distinct row indices")
        init = torch.tensor(host, dtype=torch.int32)
    gram = update_gram(clients, base)
    if clients.is_cuda:
        dev = clients.device
        if init is not None:
            init = init.to(device=dev, dtype=torch.int32)
        labels = torch.empty(K, dtype=torch.int32, device=dev)
        counts = torch.empty(C, dtype=torch.int32, device=dev)
        inertia = torch.empty((), dtype=torch.float64, device=dev)
        n_iter = torch.empty((), dtype=torch.int32, device=dev)
        with _nvq.device_guard(dev):
            _nvq.cluster_gram_kmeans(gram, K, C, init, max_iter, labels, counts, inertia, n_iter)
        return ClusterResult(labels, counts, inertia, n_iter, gram)
    u = (clients.double() - (base.double().view(1, n) if base is not None else 0.0)).numpy()
    seeds = init.numpy() if init is not None else _farthest_first(gram.numpy(), C)
    labels, counts, inertia, n_iter, _ = _lloyd(u, C, init=seeds, max_iter=max_iter)
    return ClusterResult(torch.from_numpy(labels), torch.from_numpy(counts), torch.tensor(inertia, dtype=torch.float64),
                         torch.tensor(n_iter, dtype=torch.int32), gram)


def aggregate_flat_clustered(clients: torch.Tensor, weights, labels, num_clusters: int, bases: Optional[torch.Tensor] = None,
                             clip_norm: Optional[float] = None, server_lr: float = 1.0, noise_std: float = 0.0, seed: int = 0,
                             offset: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One FedAvg step per cluster: ``out[c] = base_c + server_lr * sum_{k: labels[k] == c} c_k (clients[k] - base_c) + noise_std *
    z_c`` as a ``(C, n)`` float32 matrix, ``c_k = weights[k] / W_c * min(1, clip_norm / (|x_k - base| + 1e-6))`` with ``W_c`` the
    weights of cluster c's members, ``z_c`` the Philox stream ``(seed, offset + c)``.  ``bases``: None (zeros), a vector (one shared
    base) or a ``(C, n)`` matrix (one base per cluster; ``out`` may be it: an in-place step of the cluster models).  ``clip_norm``
    needs a shared base.  An empty cluster's row is its base (plus noise); a label outside ``[0, C)`` leaves that client out.

    On the GPU: ``nvq_fed_delta_norms`` (only with ``clip_norm``) and one ``nvq_fed_aggregate_clusters`` that reads every client row
    once; ``weights`` (float64) and ``labels`` (int32) given as device tensors are used as they are and nothing is read back.
    CPU tensors take the same formula in float64 torch operations."""
    check_clients(clients)
    K, n = clients.shape
    C = int(num_clusters)
    if not 1 <= C <= _nvq.CLUSTER_MAX:
        raise ValueError(f"num_clusters: 1 .. {_nvq.CLUSTER_MAX}")
    shared = bases is None or bases.dim() == 1
    if bases is not None and tuple(bases.shape) not in ((n,), (C, n)):
        raise ValueError("bases: a vector of n floats or a (C, n) matrix")
    if clip_norm is not None and not shared:
        raise ValueError("clip_norm needs one shared base: per-cluster bases have no single update norm")
    dev, host = clients.device, None
    if not isinstance(weights, torch.Tensor):          # zeros are fine here (a cluster may be empty): not host_weights' contracts
        host = [float(w) for w in weights]
        if len(host) != K or any(w < 0 for w in host):
            raise ValueError("weights: K non-negative numbers")
    if not isinstance(labels, torch.Tensor):
        labels = torch.tensor([int(v) for v in labels], dtype=torch.int32)
    weights = device_weights(weights, host, dev).to(device=dev, dtype=torch.float64)
    if labels.numel() != K or weights.numel() != K:
        raise ValueError("labels and weights: one per client")
    labels = labels.to(device=dev, dtype=torch.int32)
    if out is None:
        out = torch.empty(C, n, dtype=torch.float32, device=dev)
    if tuple(out.shape) != (C, n) or out.dtype != torch.float32:
        raise ValueError("out: a (C, n) float32 matrix")
    if clients.is_cuda:
        with _nvq.device_guard(dev):
            sq = None
            if clip_norm is not None:
                sq = torch.empty(K, dtype=torch.float64, device=dev)
                _nvq.fed_delta_norms(clients, n, bases, sq, _engine.workspace(dev))
            _nvq.fed_aggregate_clusters(clients, n, labels, C, bases, weights, sq, out, clip_norm=clip_norm or 0.0,
                                        server_lr=server_lr, noise_std=noise_std, seed=seed, offset=offset)
        return out
    x = clients.double()
    rows = torch.empty(C, n, dtype=torch.float32)      # every base is read before out, which may be it, is written
    for c in range(C):
        b = torch.zeros(n, dtype=torch.float64) if bases is None else (bases if shared else bases[c]).double()
        member = labels == c
        v = b
        if bool(member.any()):
            d = x[member] - b.view(1, n)
            w = weights[member]
            coef = w / w.sum()
            if clip_norm is not None:
                coef = coef * torch.clamp(clip_norm / (d.pow(2).sum(1).sqrt() + 1e-6), max=1.0)
            v = b + server_lr * (coef.view(-1, 1) * d).sum(0)
        finish_cpu(v, noise_std, seed, offset + c, rows[c])
    out.copy_(rows)
    return out


# ----------------------------------------------------------------------------------------------- the reference's names
@dataclass
class UserProfile:
    """What is known about one user: ``content_preferences`` maps a content type to the time watched, ``quality_preference`` runs
    from 0 (save battery) to 1 (best quality), ``network_pattern`` is "wifi", "cellular" or "mixed", ``device_tier`` "low", "mid" or
    "high"; ``update_vector`` may hold the user's last model update."""
    user_id: str
    content_preferences: Dict[str, float]
    quality_preference: float
    network_pattern: str
    device_tier: str
    update_vector: Optional[np.ndarray] = None


class UserClustering:
    """Cluster users by viewing behaviour (``update_clusters``, host work on the 8-feature profile vectors) or by model update
    (``cluster_updates``, on the client matrix) for personalisation."""

    CONTENT_TYPES = ("sports", "animation", "movie", "news", "music")
    NETWORK_MAP = {"wifi": 0.0, "cellular": 1.0, "mixed": 0.5}
    TIER_MAP = {"low": 0.0, "mid": 0.5, "high": 1.0}

    def __init__(self, num_clusters: int = 8, method: str = "kmeans", update_frequency: int = 10):
        if method != "kmeans":
            raise ValueError(f"method {method!r}: only 'kmeans'")
        self.num_clusters = num_clusters
        self.method = method
        self.update_frequency = update_frequency
        self.users: Dict[str, UserProfile] = {}
        self.clusters: Dict[int, List[str]] = {i: [] for i in range(num_clusters)}
        self.cluster_models: Dict[int, torch.Tensor] = {}
        self.clusterer = None

    def _fill(self, user_ids: Sequence[str], labels: Sequence[int]) -> None:
        """replace the partition: ``clusters[c]`` lists the users labelled c, in the order given"""
        fresh: Dict[int, List[str]] = {c: [] for c in range(self.num_clusters)}
        for uid, c in zip(user_ids, labels):
            fresh[int(c)].append(uid)
        self.clusters = fresh

    def register_user(self, profile: UserProfile) -> int:
        """Store the profile and put the user into a cluster, which is returned.  Once ``update_clusters`` has fitted, that is the
        nearest centroid; before, users are dealt round-robin: the user count after the insertion, modulo ``num_clusters``."""
        uid = profile.user_id
        self.users[uid] = profile
        if self.clusterer is None:
            where = len(self.users) % self.num_clusters
        else:
            where = int(self.clusterer.predict(self._extract_features(profile)[None, :])[0])
        self.clusters[where].append(uid)
        return where

    def _extract_features(self, profile: UserProfile) -> np.ndarray:
        """[sports, animation, movie, news, music watch time, quality preference, network code, device tier code]"""
        features = [profile.content_preferences.get(ct, 0.0) for ct in self.CONTENT_TYPES]
        features.append(profile.quality_preference)
        features.append(self.NETWORK_MAP.get(profile.network_pattern, 0.5))
        features.append(self.TIER_MAP.get(profile.device_tier, 0.5))
        return np.array(features, dtype=np.float64)

    RESTARTS = 4       # seeded k-means++ starts 42, 43, ...; the fit with the lowest inertia is kept (the earliest on a tie)

    def update_clusters(self) -> None:
        """Fit the profile vectors of every registered user and rebuild ``clusters`` (a no-op while there are fewer users than
        clusters)."""
        if len(self.users) < self.num_clusters:
            return
        order = list(self.users)
        X = np.stack([self._extract_features(self.users[u]) for u in order])
        fits = [_lloyd(X, self.num_clusters, seed=42 + r) for r in range(self.RESTARTS)]
        labels, counts, _, _, centers = min(fits, key=lambda f: f[2])
        self.clusterer = _HostKMeans(labels, centers, counts)
        self._fill(order, labels)

    def cluster_updates(self, user_ids: Sequence[str], clients: torch.Tensor, base: Optional[torch.Tensor] = None) -> ClusterResult:
        """Fill ``clusters`` from the users' model updates: row k of ``clients`` is user ``user_ids[k]``'s weight vector, ``base``
        the weights they started from.  The labels are copied to the host once (the only synchronisation); the returned
        ``ClusterResult`` stays on the clients' device."""
        if len(user_ids) != clients.shape[0]:
            raise ValueError("one user id per client row")
        res = cluster_updates(clients, min(self.num_clusters, clients.shape[0]), base=base)
        self._fill(user_ids, res.labels.tolist())
        return res

    def get_cluster(self, user_id: str) -> int:
        """The cluster that lists the user (the lowest one if several do); a user nobody registered gets 0, as in the reference."""
        owner: Dict[str, int] = {}
        for c in sorted(self.clusters):
            for uid in self.clusters[c]:
                owner.setdefault(uid, c)
        return owner.get(user_id, 0)

    def get_cluster_stats(self) -> Dict[int, Dict]:
        """``{cluster: {"size", "avg_quality_pref", "content_mix"}}``, non-empty clusters only: the member count, the mean
        ``quality_preference`` and the content type with the largest summed watch time ("unknown" when nobody watched anything)."""
        out: Dict[int, Dict] = {}
        for c, members in self.clusters.items():
            known = [self.users[u] for u in members if u in self.users]
            if members:
                quality = sum(p.quality_preference for p in known) / len(known) if known else 0.0
                out[c] = {"size": len(members), "avg_quality_pref": float(quality), "content_mix": self._get_dominant_content(known)}
        return out

    def _get_dominant_content(self, profiles: Sequence[UserProfile]) -> str:
        watched: Counter = Counter()
        for p in profiles:
            watched.update(p.content_preferences)
        top = watched.most_common(1)
        return top[0][0] if top else "unknown"
