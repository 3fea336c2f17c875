"""The federated client of the reference (reference nerve_cl/federated/client.py): parameters as lists of numpy arrays in
``state_dict()`` order, local training with AdamW, clipping when differential privacy is enabled.  ``VideoEnhancementClient`` is a
``flwr.client.NumPyClient`` when ``flwr`` imports and a plain class with the same methods otherwise."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

from nerve_cl import ops

try:                                                    # the transport only: nothing below needs it
    from flwr.client import NumPyClient as _ClientBase
except ImportError:
    _ClientBase = object

__all__ = ["get_parameters", "set_parameters", "VideoEnhancementClient", "create_client"]


def get_parameters(model: nn.Module) -> "List[np.ndarray]":
    """every tensor of ``model.state_dict()``, in its order, as a numpy array of its own (a CPU model's are not views of it)"""
    return [v.detach().cpu().numpy().copy() for v in model.state_dict().values()]


def set_parameters(model: nn.Module, parameters: "List[np.ndarray]") -> None:
    """the inverse of ``get_parameters``; the values are copied in place (``load_state_dict(strict=True)``), so the flat parameter
    buffer of a HIP-backed network stays where it is"""
    keys = list(model.state_dict().keys())
    if len(keys) != len(parameters):
        raise ValueError(f"{len(parameters)} arrays for a state dict of {len(keys)} tensors")
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in zip(keys, parameters)}, strict=True)


class VideoEnhancementClient(_ClientBase):
    """Local training on one user's data: ``fit`` loads the given parameters, runs ``local_epochs`` of AdamW over ``train_loader``
    with the MSE criterion and - ``dp_enabled`` - global-norm clipping to ``dp_max_grad_norm`` before every step, and returns
    ``(parameters, samples seen, {"train_loss": mean loss per sample})``."""

    def __init__(self, model: nn.Module, train_loader: DataLoader, val_loader: Optional[DataLoader] = None, device: str = "cpu",
                 local_epochs: int = 5, learning_rate: float = 1e-4, dp_enabled: bool = True, dp_epsilon: float = 8.0,
                 dp_max_grad_norm: float = 1.0):
        self.model = model.to(device)
        self.train_loader = train_loader
        self.val_loader = val_loader
        self.device = device
        self.local_epochs = local_epochs
        self.learning_rate = learning_rate
        self.dp_enabled = dp_enabled
        self.dp_epsilon = dp_epsilon
        self.dp_max_grad_norm = dp_max_grad_norm
        self.criterion = nn.MSELoss()

    def get_parameters(self, config: Dict) -> "List[np.ndarray]":
        return get_parameters(self.model)

    def fit(self, parameters: "List[np.ndarray]", config: Dict) -> "Tuple[List[np.ndarray], int, Dict]":
        set_parameters(self.model, parameters)
        epochs = config.get("local_epochs", self.local_epochs)
        optimizer = torch.optim.AdamW(self.model.parameters(), lr=self.learning_rate)
        self.model.train()
        total, seen = 0.0, 0
        for _ in range(epochs):
            for batch in self.train_loader:
                inputs, targets = batch[0].to(self.device), batch[1].to(self.device)
                optimizer.zero_grad()
                loss = self.criterion(self.model(inputs), targets)
                loss.backward()
                if self.dp_enabled:
                    ops.clip_grad_norm_(self.model, self.dp_max_grad_norm)
                optimizer.step()
                total += loss.item() * inputs.size(0)
                seen += inputs.size(0)
        return get_parameters(self.model), seen, {"train_loss": total / max(seen, 1)}

    def evaluate(self, parameters: "List[np.ndarray]", config: Dict) -> "Tuple[float, int, Dict]":
        set_parameters(self.model, parameters)
        if self.val_loader is None:
            return 0.0, 0, {}
        self.model.eval()
        total, seen = 0.0, 0
        with torch.no_grad():
            for batch in self.val_loader:
                inputs, targets = batch[0].to(self.device), batch[1].to(self.device)
                loss = self.criterion(self.model(inputs), targets)
                total += loss.item() * inputs.size(0)
                seen += inputs.size(0)
        avg = total / max(seen, 1)
        return avg, seen, {"val_loss": avg}


def create_client(client_id: int, model: nn.Module, train_data, val_data=None, **kwargs) -> VideoEnhancementClient:
    """a client over ``(inputs, targets)`` tensors in batches of 16 (reference client.py:137-160)"""
    train_loader = DataLoader(TensorDataset(train_data[0], train_data[1]), batch_size=16, shuffle=True)
    val_loader = DataLoader(TensorDataset(val_data[0], val_data[1]), batch_size=16) if val_data is not None else None
    return VideoEnhancementClient(model=model, train_loader=train_loader, val_loader=val_loader, **kwargs)
