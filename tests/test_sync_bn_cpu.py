"""CPU: enable_data_parallel(sync_bn=True) converts every BatchNorm holder of the HIP networks to nn.SyncBatchNorm without
changing the state_dict, and a sub-module replaced after construction drops the network's cached slots, bucket layout and
synchronised-BatchNorm list (no process group here: the conversion itself is what is checked)."""
import pytest
import torch
import torch.nn as nn

from nerve_cl import parallel
from nerve_cl.models import FrameRecoveryNet, LightweightSuperResolution, SuperResolutionNet

NETS = [(lambda: SuperResolutionNet(3, 2, 16, 1, 1), 3), (lambda: LightweightSuperResolution(2), 4),
        (lambda: FrameRecoveryNet(3, 16, 2), 29)]


def _bn_count(net, kind):
    return sum(isinstance(m, kind) for m in net.modules())


@pytest.mark.parametrize("make,n_bn", NETS)
def test_sync_bn_converts_every_holder(make, n_bn):
    net = make()
    plain = _bn_count(net, nn.modules.batchnorm._BatchNorm)
    assert plain == n_bn and _bn_count(net, nn.SyncBatchNorm) == 0
    out = parallel.enable_data_parallel(net, sync_bn=True)
    assert out is net
    assert _bn_count(net, nn.SyncBatchNorm) == n_bn
    assert _bn_count(net, nn.modules.batchnorm._BatchNorm) == n_bn


@pytest.mark.parametrize("make,n_bn", NETS)
def test_sync_bn_state_dict_unchanged_and_loads_both_ways(make, n_bn):
    torch.manual_seed(1)
    ref = make()
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    conv = parallel.enable_data_parallel(make(), sync_bn=True)
    sd2 = conv.state_dict()
    assert list(sd2) == list(sd)
    for k, v in sd.items():
        assert sd2[k].shape == v.shape and sd2[k].dtype == v.dtype, k
    conv.load_state_dict(sd)
    for k, v in conv.state_dict().items():
        assert torch.equal(v, sd[k]), k
    back = make()
    back.load_state_dict(conv.state_dict())
    for k, v in back.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_sync_bn_default_leaves_holders_alone():
    net = SuperResolutionNet(3, 2, 16, 1, 1)
    parallel.enable_data_parallel(net)
    assert _bn_count(net, nn.SyncBatchNorm) == 0
    assert net._sync_bn_groups() == {}


@pytest.mark.parametrize("make,n_bn", NETS)
def test_caches_follow_a_conversion(make, n_bn):
    net = make()
    slots_before = net._slots()
    net._bucket_layout()
    assert net._sync_bn_groups() == {}                      # builds the (empty) holder list
    assert net.__dict__["_sync_cache"] == []
    nn.SyncBatchNorm.convert_sync_batchnorm(net)             # add_module on every child of the network
    assert "_slot_cache" not in net.__dict__ and "_sync_cache" not in net.__dict__ and net._layout is None
    assert net._sync_bn_groups() == {}                       # not initialised: the unsynchronised path
    assert len(net.__dict__["_sync_cache"]) == n_bn
    # the slots now point at the converted holders' parameter / buffer dicts
    owners = {id(m._parameters): m for m in net.modules()}
    for name, d, key in net._slots()[0]:
        assert id(d) in owners and d[key] is net.get_parameter(name), name
    assert len(net._slots()[0]) == len(slots_before[0])
    assert net._param_names == [n for n, _ in net.named_parameters()]


def test_setattr_replacing_a_submodule_invalidates():
    net = SuperResolutionNet(3, 2, 16, 1, 1)
    net._slots()
    net._bucket_layout()
    net._sync_bn_groups()
    body = net.feature_extractor.body
    net.feature_extractor = nn.SyncBatchNorm.convert_sync_batchnorm(net.feature_extractor)
    assert "_slot_cache" not in net.__dict__ and "_sync_cache" not in net.__dict__ and net._layout is None
    net._sync_bn_groups()
    assert len(net.__dict__["_sync_cache"]) == 3
    assert net.feature_extractor.body is not body or _bn_count(body, nn.SyncBatchNorm) == 3
    # a plain attribute (not a module) keeps the caches
    net._slots()
    net.some_flag = True
    assert "_slot_cache" in net.__dict__
