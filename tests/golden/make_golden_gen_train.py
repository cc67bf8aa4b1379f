"""Writes tests/golden/gen_train_{a,b}.npz (with gen_train_b_<i>.npz and gen_train_c.npz) from the REFERENCE's own ``decoder.Generator`` (CPU, torch autograd, the module in ``.double()``).

Run once on the build machine (needs the reference checkout, ``I2V_REFERENCE``; never runs on the GPU machine):

    I2V_REFERENCE=/path/to/reference python tests/golden/make_golden_gen_train.py [--check]

``Spade.forward`` hard-codes ``.cuda()`` (normalization_layer.py:20); on a GPU-less host ``Tensor.cuda`` is made the identity before the
reference is imported, as make_golden.py does.

Per fixture of ``gen_train_common.FIXTURES`` (parameters and inputs are seeded numpy draws that the tests regenerate, not stored), the module
in ``.train()`` mode and the loss sum(c frames), all float64:
  {tag}.out, {tag}.dz                     the frames [B, T, 3, H, W] and motion.grad
  {tag}.g.<key>                           the gradients of fc.bias, conv_img.weight, conv_img.bias and of every block's conv_0.bias in full
  {tag}.n.<key>, {tag}.p.<key>            every other parameter's gradient: its norm and its inner products with N_DIRECTIONS seeded
                                          unit directions (the full gradients are about 36 MB)
  {tag}.sgd_losses, _f32, .sgd_scale      the loss before each of SGD_STEPS plain SGD steps (lr ``SGD_LR``) in float64 and in fp32, and
                                          sum |c frames| per step, the scale the loss is compared on
  {case}.d32.<tensor>                     for ``out``, ``dz`` and every ``g.<key>``, of all three cases (case c has nothing else, in
                                          gen_train_c.npz): the relative L2 distance of the reference's own fp32 run from its float64
                                          run (the zero gradients on their own scale), from which gen_train_common.gate_of takes the gate
An array of more than 700 KB (case b's frames) is cut into files of its own, which load_golden joins again.
``--check`` writes nothing.  Either way the run prints those distances and how many lie above a quarter of the 1e-4 gate (the frames must
not), prints the 99th percentile of the pre-tanh values and asserts that it stays below 2, and prints the SGD losses' fp32 / float64
distance at this learning rate.  Results only, never text."""
import argparse
import os
import sys

import numpy as np
import torch

torch.Tensor.cuda = lambda self, *a, **k: self  # see the docstring

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gen_train_common as gt  # noqa: E402


def ref_module(case, sd, dtype):
    sys.path.insert(0, os.environ["I2V_REFERENCE"])
    from stage1_VAE.modules.decoder import Generator
    m = Generator(gt.dic_of(case))
    own = m.state_dict()
    assert {k: tuple(v.shape) for k, v in own.items()} == gt.param_shapes(case)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dtype).train()


def run(case, sd, dtype):
    img, z, c = (t.to(dtype) for t in gt.inputs(case))
    m = ref_module(case, sd, dtype)
    pre = []
    m.conv_img.register_forward_hook(lambda mod, i, o: pre.append(o.detach()))
    z.requires_grad_(True)
    out = m(img, z)
    (c * out).sum().backward()
    res = {"out": out.detach().contiguous(), "dz": z.grad, "pre": pre[0]}
    for k, p in m.named_parameters():
        res["g." + k] = p.grad
    return res


def sgd(case, sd, dtype):
    img, z, c = (t.to(dtype) for t in gt.inputs(case))
    m = ref_module(case, sd, dtype)
    losses, scale = [], []
    for _ in range(gt.SGD_STEPS):
        m.zero_grad()
        out = m(img, z)
        loss = (c * out).sum()
        loss.backward()
        losses.append(float(loss))
        scale.append(float((c * out).abs().sum()))
        with torch.no_grad():
            for p in m.parameters():
                p -= gt.SGD_LR * p.grad
    return np.array(losses), np.array(scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="print the distances, write nothing")
    ap.add_argument("--no-sgd", action="store_true", help="skip the SGD sequences (with --check)")
    args = ap.parse_args()
    for tag in sorted(gt.CASES):
        case = gt.CASES[tag]
        sd = gt.synthetic_state(case)
        r64, r32 = run(case, sd, torch.float64), run(case, sd, torch.float32)
        p99 = float(np.quantile(r64["pre"].abs().numpy(), 0.99))
        print(f"case {tag}: pre-tanh |pre| 99th percentile {p99:.3f}, max {float(r64['pre'].abs().max()):.3f}")
        assert p99 < 2.0, p99
        img, z, c = gt.inputs(case)
        scale = gt.generator(sd, img, z, case, c)["scale"]
        store, worst, over = {}, (0.0, ""), 0
        for k in (k for k in r64 if k != "pre"):
            d = gt.rel(r32[k], r64[k], scale.get(k[2:]))
            print(f"  {k}: the reference's fp32 run against its float64 run, rel-L2 {d:.2e}")
            worst, over = max(worst, (d, k)), over + (d > gt.TOL_L2 / 4)
            store[f"{tag}.d32.{k}"] = np.float64(d)
            if tag not in gt.FIXTURES:
                continue
            v = r64[k].detach().numpy()
            key = k[2:]
            if not k.startswith("g.") or key in gt.FULL_GRADS or gt.is_zero_grad(key):
                store[f"{tag}.{k}"] = v
            else:
                store[f"{tag}.n.{key}"], store[f"{tag}.p.{key}"] = gt.summary(key, v)
        print(f"case {tag}: worst rel-L2 {worst[0]:.2e} ({worst[1]}); {over} of {len(r64) - 1} tensors lie above the gate / 4 = {gt.TOL_L2 / 4:.1e}")
        assert gt.rel(r32["out"], r64["out"]) <= gt.TOL_L2 / 4
        if not args.no_sgd and tag in gt.FIXTURES:
            l64, s64 = sgd(case, sd, torch.float64)
            l32, _ = sgd(case, sd, torch.float32)
            dist = np.abs(l32 - l64) / s64
            print(f"fixture {tag}: SGD lr {gt.SGD_LR}: losses {l64}, |fp32 - float64| / scale {dist}")
            assert len(set(np.round(l64, 6))) == gt.SGD_STEPS
            store[f"{tag}.sgd_losses"], store[f"{tag}.sgd_losses_f32"], store[f"{tag}.sgd_scale"] = l64, l32, s64
        if not args.check:
            # every committed file stays below 1 MiB: an array of more than 700 KB (case b's frames) is cut along its second axis into
            # pieces "<key>@<i>" with a file each (gen_train_<tag>_<i>.npz), which gen_train_common.load_golden joins again
            files = [{}]
            for k, v in store.items():
                v = np.asarray(v)
                if v.nbytes <= 700_000:
                    files[0][k] = v
                else:
                    for i, piece in enumerate(np.array_split(v, -(-v.nbytes // 700_000), axis=1)):
                        files.append({f"{k}@{i}": piece})
            for i, part in enumerate(files):
                path = os.path.join(HERE, f"gen_train_{tag}.npz" if i == 0 else f"gen_train_{tag}_{i}.npz")
                np.savez_compressed(path, **part)
                print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
