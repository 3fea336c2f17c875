"""Federated learning with differential privacy: the reference's ``nerve_cl.federated`` names on the flat parameter and gradient
buckets (csrc/federated.hip), and user clustering for personalised models on the client matrix
(csrc/cluster.hip), and Byzantine-robust aggregation of that matrix: trimmed mean, median, Krum
(csrc/robust.hip), and federated optimisation for clients that differ: the FedOpt server rules and the FedProx
gradient (csrc/fedopt.hip), and compressed client updates: top-k with error feedback and QSGD quantisation
(csrc/compress.hip).  The ``flwr`` transport is not part of it."""
from nerve_cl.federated.client import VideoEnhancementClient, create_client, get_parameters, set_parameters
from nerve_cl.federated.compression import COMPRESSIONS, compress_updates_, topk_count, wire_bytes
from nerve_cl.federated.clustering import (ClusterResult, UserClustering, UserProfile, aggregate_flat_clustered, cluster_updates,
                                           update_gram, update_similarity)
from nerve_cl.federated.fedopt import SERVER_OPTIMIZERS, ServerOptimizer, prox_grad_
from nerve_cl.federated.privacy import (DPOptimizer, PrivacyConfig, compute_noise_multiplier, get_privacy_spent, make_private)
from nerve_cl.federated.robust import (KrumResult, aggregate_flat_median, aggregate_flat_trimmed, krum_aggregate_flat,
                                       krum_select)
from nerve_cl.federated.trainer import FederatedTrainer, aggregate_flat, fedavg, start_server, weighted_average

__all__ = ["VideoEnhancementClient", "create_client", "get_parameters", "set_parameters", "FederatedTrainer", "start_server",
           "weighted_average", "fedavg", "aggregate_flat", "PrivacyConfig", "DPOptimizer", "make_private",
           "compute_noise_multiplier", "get_privacy_spent", "UserProfile", "UserClustering", "ClusterResult", "update_gram",
           "update_similarity", "cluster_updates", "aggregate_flat_clustered", "KrumResult", "aggregate_flat_trimmed",
           "aggregate_flat_median", "krum_select", "krum_aggregate_flat", "SERVER_OPTIMIZERS", "ServerOptimizer", "prox_grad_",
           "compress_updates_", "topk_count", "wire_bytes", "COMPRESSIONS"]
