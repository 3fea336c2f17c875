"""GPU: the continual-learning consumers of the SR hot path through the PRODUCT classes on the HIP
network, against numbers captured from the reference's own classes (oracle/make_goldens.py --only-cl):

 * nerve_cl.continual.FOMAML.adapt / Reptile.train_step vs tests/golden/meta_f16.npz (reference maml.py:74-110,168-186,276-345),
 * nerve_cl.continual.SynapticIntelligence (flat-bucket kernels nvq_si_update / nvq_si_consolidate) vs si_f16.npz
   (reference ewc.py:306-379),
 * the `mse + ewc.penalty()` loop of experiments/train_continual.py:26-69 with the product EWC (penalty gradient fused into the
   gradient bucket) vs cfg5_loop.npz: per-step task_loss / ewc_loss and the final Fisher,
 * experiments/train_continual.py --strategy ewc as a process.
The inputs are the closed-form ones of oracle/cl_cases.py; exact-fp32 kernels (the package's default math mode), and the cfg5
loop once more in the mode the script defaults to (bf16 + graph replay) with bf16 tolerances."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cl_cases
from oracle.make_goldens import Adapter4D, delta_summaries, grad_summary

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net():
    from nerve_cl.models import SuperResolutionNet
    c = cl_cases.META
    net = SuperResolutionNet(3, c["s"], c["F"], c["N"], c["win"])
    net.load_state_dict(cl_cases.state())
    return net.cuda().train()


def _cuda(pair):
    return pair[0].cuda(), pair[1].cuda()


def _summ_close(got, ref, what, tol):
    err = np.abs(np.asarray(got) - np.asarray(ref)).max() / max(abs(ref[1]), 1e-30)
    assert err <= tol, f"{what}: {err:.3e}"


def _mse():
    from nerve_cl import ops
    return ops.mse_loss                 # the loops' nn.MSELoss as libnvq kernels


def test_fomaml_adapt_and_reptile_train_step_match_the_reference(golden_dir):
    from nerve_cl.continual import FOMAML, Reptile
    g = np.load(os.path.join(golden_dir, "meta_f16.npz"))
    fo, rp = cl_cases.FOMAML, cl_cases.REPTILE
    names = [k[len("fomaml_delta/"):] for k in g.files if k.startswith("fomaml_delta/")]
    net = _net()
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    assert sorted(before) == sorted(names)
    data = _cuda(cl_cases.clip_pair(fo["data_seed"]))
    adapted = FOMAML(net, inner_lr=fo["inner_lr"], inner_steps=fo["steps"]).adapt(data, _mse())
    assert adapted is not net and all(torch.equal(p, before[n]) for n, p in net.named_parameters())
    d = delta_summaries({n: v.cpu() for n, v in before.items()}, {n: p.cpu() for n, p in adapted.named_parameters()})
    for n in names:
        _summ_close(d[n], g["fomaml_delta/" + n], "fomaml " + n, 5e-3)
    adapted.eval()
    with torch.no_grad():
        assert abs(_mse()(adapted(data[0]), data[1]).item() - float(g["fomaml_eval_loss"])) < 2e-5
    sd = adapted.state_dict()
    for k in g.files:
        if k.startswith("fomaml_buf/"):
            ref = g[k].astype(np.float64)
            assert np.abs(sd[k[len("fomaml_buf/"):]].cpu().double().numpy() - ref).max() <= 1e-4 * max(np.abs(ref).max(), 1e-30), k

    net = _net()
    before = {n: p.detach().clone().cpu() for n, p in net.named_parameters()}
    tasks = [{"support": _cuda(cl_cases.clip_pair(s))} for s in rp["data_seeds"]]
    loss = Reptile(net, inner_lr=rp["inner_lr"], outer_lr=rp["outer_lr"], inner_steps=rp["inner_steps"]).train_step(tasks, _mse())
    assert abs(loss - float(g["reptile_loss"])) < 2e-5
    d = delta_summaries(before, {n: p.cpu() for n, p in net.named_parameters()})
    for n in names:
        _summ_close(d[n], g["reptile_delta/" + n], "reptile " + n, 5e-3)
    sd = net.state_dict()
    for k in g.files:
        if k.startswith("reptile_buf/"):
            ref = g[k].astype(np.float64)
            assert np.abs(sd[k[len("reptile_buf/"):]].cpu().double().numpy() - ref).max() <= 1e-4 * max(np.abs(ref).max(), 1e-30), k


def test_synaptic_intelligence_on_the_flat_bucket_matches_the_reference(golden_dir):
    from nerve_cl.continual import SynapticIntelligence
    g = np.load(os.path.join(golden_dir, "si_f16.npz"))
    net = _net()
    si = SynapticIntelligence(net, si_lambda=cl_cases.SI["si_lambda"], damping=cl_cases.SI["damping"])
    names = [k[2:] for k in g.files if k.startswith("W/")]
    assert sorted(si.W) == sorted(names)
    x, t = _cuda(cl_cases.si_pair())
    W, omega, pens, losses = cl_cases.si_drive(net, si, names, x, t, _mse())
    assert np.allclose(losses, g["losses"], rtol=2e-5)
    assert pens[:3] == [0.0, 0.0, 0.0]                         # the reference's p_old quirk, kept
    assert np.allclose(pens[3:], g["penalties"][3:], rtol=1e-2)
    for n in names:
        _summ_close(grad_summary(W[n].cpu()), g["W/" + n], "W " + n, 1e-2)
        _summ_close(grad_summary(omega[n].cpu()), g["omega/" + n], "omega " + n, 1e-2)
    # after a plain zero_grad -> backward -> step the .grad tensors ARE the views of the network's gradient bucket, i.e.
    # update_importance is the one-launch path (a backward that also accumulated a separately returned penalty gradient,
    # like the last steps of si_drive, replaces .grad by a sum and takes the per-tensor path)
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    opt.zero_grad()
    _mse()(net(x), t).backward()
    opt.step()
    assert all(si._segs[0].net.grad_alias_mask() or [False])
    w0 = si._W[0].clone()
    si.update_importance()
    assert not torch.equal(w0, si._W[0]) and torch.equal(si._p_old[0], net.flat_theta())


def _run_cfg5_loop(net):
    """experiments/train_continual.py:26-69 with reference semantics: Adam(1e-4), loss = mse + penalty, register_task per
    task - the product EWC around the HIP network through the 4-D -> 5-D adapter.  -> (task losses, ewc losses, EWC)"""
    from nerve_cl.continual import EWC
    model = Adapter4D(net)
    ewc = EWC(model, ewc_lambda=cl_cases.CFG5["lam"])
    opt = torch.optim.Adam(model.parameters(), lr=cl_cases.CFG5["lr"])
    crit = _mse()
    tl, el = [], []
    for task_id, (_, batches) in enumerate(cl_cases.cfg5_tasks()):
        batches = [(a.cuda(), b.cuda()) for a, b in batches]
        model.train()
        for lr_b, hr_b in batches:
            opt.zero_grad()
            task_loss = crit(model(lr_b), hr_b)
            ewc_loss = ewc.penalty()
            (task_loss + ewc_loss).backward()
            opt.step()
            tl.append(task_loss.item())
            el.append(float(ewc_loss.item()) if torch.is_tensor(ewc_loss) else float(ewc_loss))
        ewc.register_task(task_id, batches)
    return tl, el, ewc


def test_train_with_ewc_loop_matches_the_reference_trajectory(golden_dir):
    g = np.load(os.path.join(golden_dir, "cfg5_loop.npz"))
    tl, el, ewc = _run_cfg5_loop(_net())
    assert np.allclose(tl, g["task_loss"], rtol=5e-5), (tl, g["task_loss"])
    assert el[:4] == [0.0] * 4
    assert np.allclose(el[4:], g["ewc_loss"][4:], rtol=2e-2), (el, g["ewc_loss"])
    for k in g.files:
        if k.startswith("fisher/"):
            _summ_close(grad_summary(ewc.fisher_dict["net." + k[7:]].cpu()), g[k], k, 5e-3)


def test_train_with_ewc_loop_in_the_scripts_default_mode(golden_dir):
    """The mode experiments/train_continual.py runs by default - configure_precision(model, "bf16", "auto"): bf16 MFMA operands,
    bf16-stored conv-internal tensors, HIP-graph replay of the step - through the same loop, against the reference's fp32
    numbers (cfg5_loop.npz) with bf16 tolerances: per-step task loss within 2e-3 (relative), EWC loss within 10 %, every
    Fisher tensor's sum within 8 % (the whole Fisher within 5 %) of the reference's and - against the exact-fp32 mode of this build, which the test above
    pins to the fixture at 5e-3 - a per-tensor cosine >= 0.99.  The reference loop is fp32 (train_continual.py:26-69,
    ewc.py:73-149): this is the statement of what the default mode's reduced precision costs."""
    import importlib.util
    import types
    sys.path.insert(0, os.path.join(REPO, "experiments"))     # (the script imports its sibling _common.py)
    spec = importlib.util.spec_from_file_location("train_continual_script", os.path.join(REPO, "experiments", "train_continual.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    g = np.load(os.path.join(golden_dir, "cfg5_loop.npz"))
    _, _, ewc32 = _run_cfg5_loop(_net())
    net = _net()
    script.configure_precision(types.SimpleNamespace(super_resolution=net), "bf16", "auto")
    tl, el, ewc = _run_cfg5_loop(net)
    assert net._step_graphs.replays > 0                        # the step really was replayed from a HIP graph
    dev_t = np.abs(np.asarray(tl) / g["task_loss"] - 1).max()
    assert dev_t <= 2e-3, (tl, g["task_loss"])
    assert el[:4] == [0.0] * 4
    dev_e = np.abs(np.asarray(el[4:]) / g["ewc_loss"][4:] - 1).max()
    assert dev_e <= 0.10, (el, g["ewc_loss"])
    rows, tot16, tot_ref = [], 0.0, 0.0
    for k in g.files:
        if not k.startswith("fisher/"):
            continue
        f16, f32 = ewc.fisher_dict["net." + k[7:]].double().flatten(), ewc32.fisher_dict["net." + k[7:]].double().flatten()
        cos = (torch.dot(f16, f32) / (f16.norm() * f32.norm()).clamp_min(1e-300)).item()
        rows.append((k[7:], cos, abs(f16.sum().item() / g[k][0] - 1)))
        tot16 += f16.sum().item()
        tot_ref += float(g[k][0])
    worst_cos, worst_sum = min(r[1] for r in rows), max(r[2] for r in rows)
    print(f"default-mode cfg5 loop vs reference: task loss {dev_t:.2e}, ewc loss {dev_e:.2e}, Fisher min cosine "
          f"{worst_cos:.5f}, worst per-tensor sum deviation {worst_sum:.2e}, total Fisher {abs(tot16 / tot_ref - 1):.2e}, "
          f"graph replays {net._step_graphs.replays}")
    for r in sorted(rows, key=lambda r: -r[2])[:5]:
        print(f"    {r[0]}: cosine {r[1]:.5f}, sum off by {r[2]:.3f}")
    assert worst_cos >= 0.99, [r for r in rows if r[1] < 0.99]
    # a Fisher entry is a squared gradient: 5 % on a tensor's sum is a 2.5 % gradient error.  Measured: task loss 8e-4, EWC loss
    # 5e-3, min cosine 0.9918, whole Fisher 0.5 %, every tensor's sum within 3.5 % except the first attention conv (bias 7.0 %,
    # weight 6.3 %: the smallest gradients of the net, formed behind the softmax from bf16-stored feature tensors); bound 8 %
    # per tensor, 5 % on the whole Fisher
    assert worst_sum <= 0.08, [r for r in rows if r[2] > 0.08]
    assert abs(tot16 / tot_ref - 1) <= 0.05


@pytest.mark.timeout(600)
def test_train_continual_ewc_strategy_as_a_process(tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable, os.path.join(REPO, "experiments", "train_continual.py"), "--strategy", "ewc", "--tasks", "2",
                        "--samples", "32", "--epochs", "2", "--features", "16", "--blocks", "1"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    out = r.stdout
    assert "=== Training on Task 0: sports ===" in out and "=== Training on Task 1: animation ===" in out
    assert out.count("Registered task") == 2 and "Training complete!" in out
    losses = [float(ln.split("Loss=")[1]) for ln in out.splitlines() if "Loss=" in ln]
    assert len(losses) == 4 and all(np.isfinite(losses))
    sd = torch.load(tmp_path / "checkpoints" / "continual_model.pt", weights_only=True)
    assert "enhancement_strength" in sd and any(k.startswith("super_resolution.residual_blocks.0.") for k in sd)
