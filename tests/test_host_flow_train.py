"""CPU-side checks of the flow-training feature: the gradient reference (oracle autograd) against the fixture made from the
reference's own autograd, FlowLoss, the exported training symbols, FusedAdam's state_dict layout, and the refusals that need
no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import i2v_synth as synth
from conftest import PKG, REPO
from flow_train_common import load_grad_fixture, oracle_grads, rel

TRAIN_SYMBOLS = ["i2v_flow_train_create", "i2v_flow_train_destroy", "i2v_flow_train_bind", "i2v_flow_train_saved_bytes", "i2v_flow_train_saved_layout",
                 "i2v_flow_train_forward", "i2v_flow_train_backward", "i2v_adam_step", "i2v_adam_chunk"]


def test_oracle_autograd_matches_reference_autograd_fixture():
    """Every tensor <= 1e-5 relative L2 (measured: <= 1.3e-7): pins the reference of the GPU gradient tests."""
    arrays, meta = load_grad_fixture()
    sd = synth.flow_state_dict(**meta["synth"])
    zt, logdet, loss, grads = oracle_grads(sd, torch.from_numpy(arrays["x"]), torch.from_numpy(arrays["embed"]), torch.float32,
                                           meta["synth"]["n_flows"], meta["synth"]["control"])
    worst = {"zt": rel(zt, arrays["zt"]), "logdet": rel(logdet, arrays["logdet"]), "loss": rel(loss, arrays["loss"]),
             "d_x": rel(grads["x"], arrays["d_x"]), "d_embed": rel(grads["embed"], arrays["d_embed"])}
    names = [k for k in sd if np.asarray(sd[k]).dtype.kind == "f"]
    assert len(names) == 68 and all("grad." + k in arrays for k in names)
    for k in names:
        worst[k] = rel(grads[k], arrays["grad." + k])
    print("worst", max(worst.values()), max(worst, key=worst.get))
    assert max(worst.values()) <= 1e-5, {k: v for k, v in worst.items() if v > 1e-5}


def test_flow_loss_formula_logger_and_no_wandb():
    from stage2_cINN.modules.loss import FlowLoss, LossLogger, nll
    arrays, _ = load_grad_fixture()
    zt = torch.from_numpy(arrays["zt"])[:, :, None, None]
    logdet = torch.from_numpy(arrays["logdet"])
    assert torch.allclose(nll(zt), 0.5 * (zt.double() ** 2).sum(dim=(1, 2, 3)).float(), rtol=1e-6)
    logger = LossLogger()
    torch.manual_seed(3)
    loss = FlowLoss()(zt, logdet, logger, mode="train")
    torch.manual_seed(3)
    ref_draw = torch.randn_like(zt)    # the loss consumes exactly this draw
    after = torch.randn(1)
    torch.manual_seed(3)
    torch.randn_like(zt)
    assert torch.equal(after, torch.randn(1))
    want = float((0.5 * (zt.double() ** 2).sum(dim=(1, 2, 3))).mean() - logdet.double().mean())
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    assert abs(float(loss) - float(arrays["loss"])) <= 1e-5 * abs(float(arrays["loss"]))
    (entry,) = logger.entries
    assert set(entry) == {"Loss", "reference_nll_loss", "nlogdet_loss", "nll_loss"}
    assert all(isinstance(v, float) for v in entry.values())
    assert abs(entry["Loss"] - (entry["nll_loss"] + entry["nlogdet_loss"])) <= 1e-4 * abs(entry["Loss"])
    assert abs(entry["reference_nll_loss"] - float(nll(ref_draw).mean())) <= 1e-6 * entry["reference_nll_loss"]
    with pytest.raises(ImportError):
        import wandb  # noqa: F401  (not installed here: the loss above ran without it)


def test_training_symbols_are_declared_and_exported():
    import i2v_native
    if not os.path.exists(i2v_native.LIB_PATH):
        i2v_native.build()
    lib = ctypes.CDLL(i2v_native.LIB_PATH)
    header = open(os.path.join(REPO, "include", "i2v_hip.h")).read()
    declared = set(re.findall(r"\b(i2v_[a-z0-9_]+)\s*\(", header))
    for name in TRAIN_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/i2v_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in i2v_native.SYMBOLS
    assert lib.i2v_adam_chunk() > 0 and lib.i2v_adam_chunk() % 4 == 0


def test_train_source_reads_no_environment():
    text = open(os.path.join(PKG, "csrc", "i2v_flow_train.hip")).read()
    assert "getenv" not in text
    assert "i2v_flow_train.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()


def _small_flow():
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    return ConditionalFlow(64, 64, 128, 2, 2, conditioning_option="None")


def test_fused_adam_state_dict_is_torch_adams():
    from i2v_train import FusedAdam
    flow = _small_flow()
    params = list(flow.parameters())
    ref = torch.optim.Adam(params, lr=1e-5, betas=(0.9, 0.99), weight_decay=0, amsgrad=True)
    for p in params:
        p.grad = torch.full_like(p, 0.25)
    ref.step()
    ref.step()
    fused = FusedAdam(params, lr=1e-5, betas=(0.9, 0.99), weight_decay=0, amsgrad=True)
    assert set(fused.state_dict()) == set(ref.state_dict())
    assert set(fused.state_dict()["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])
    fused.load_state_dict(ref.state_dict())
    sd = fused.state_dict()
    assert len(sd["state"]) == len(params)
    for i, st in sd["state"].items():
        assert set(st) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
        assert float(st["step"]) == 2.0 and torch.equal(st["exp_avg"], ref.state_dict()["state"][i]["exp_avg"])
    # ... and back: torch's Adam takes FusedAdam's state dict and steps on it
    back = torch.optim.Adam(params, lr=1e-3)
    back.load_state_dict(sd)
    back.step()
    assert float(back.state_dict()["state"][0]["step"]) == 3.0 and back.param_groups[0]["lr"] == 1e-5
    sched = torch.optim.lr_scheduler.StepLR(fused, step_size=1, gamma=0.5)
    sched.step()
    assert fused.param_groups[0]["lr"] == pytest.approx(5e-6)
    # parameters without .grad are skipped like torch skips them; the rest would need a GPU, and there is no CPU fallback
    for p in params:
        p.grad = None
    FusedAdam(params).step()
    params[0].grad = torch.zeros_like(params[0])
    import i2v_native
    with pytest.raises(i2v_native.I2VError):
        FusedAdam(params).step()


def test_differentiable_flag_default_state_dict_and_cpu_refusal():
    import i2v_native
    from stage2_cINN.modules.INN import SupervisedTransformer
    flow = _small_flow()
    keys = set(flow.state_dict())
    assert flow.differentiable is False
    flow.differentiable = True
    assert set(flow.state_dict()) == keys and "differentiable" not in dict(flow.named_buffers())
    flow.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in
                          synth.flow_state_dict(seed=7, n_flows=2, embedding_dim=64, hidden_dim=128).items()})
    with torch.enable_grad(), pytest.raises(i2v_native.I2VError):
        flow(torch.randn(3, 64), torch.randn(3, 64))     # a module on the CPU raises: no eager fallback
    net = SupervisedTransformer(flow_in_channels=64, flow_mid_channels=128, flow_hidden_depth=2, n_flows=2,
                                flow_conditioning_option="None", control=False)
    assert net.differentiable is False
    net.differentiable = True
    assert net.flow.differentiable is True and set(net.state_dict()) == {"flow." + k for k in net.flow.state_dict()}
