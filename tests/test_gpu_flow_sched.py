"""GPU checks of the cINN host code around the pass schedule (csrc/i2v_flow_sched.h): every skip_actnorm / skip_shuffle / activation
combination at TWO blocks (the schedule's block-boundary branches need a boundary; the module mirrors exercise these flags at
n_flows = 1 only) on every launch chain, and the one graph cache (run_chain in csrc/i2v_flow.hip) against eager launches."""
import itertools

import numpy as np
import pytest
import torch

import i2v_synth as synth
from conftest import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-4                                   # the project's parity gate (tests/test_gpu_parity.py)
HID, DEPTH, EMB, NFL = 128, 1, 64, 2         # the smallest geometry the tile chain covers, two blocks
FLAGS = list(itertools.product((False, True), (False, True), ("lrelu", "none")))   # skip_actnorm, skip_shuffle, activation
CHAINS = {"folded": ("I2V_FLOW_FOLD", "1"), "unfolded": ("I2V_FLOW_FOLD", "0"), "generic": ("I2V_FLOW_TILE", "0")}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import i2v_native
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    i2v_native.lib()
    torch.set_grad_enabled(False)


def T(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _handle(monkeypatch, chain, sd, skip_an=False, skip_sh=False, act="lrelu", use_graph=True):
    """A NativeFlow on the named chain: the switches are read at create (I2V_FLOW_TILE) and at load (I2V_FLOW_FOLD) only."""
    import i2v_native
    var, val = CHAINS[chain]
    monkeypatch.setenv(var, val)
    h = i2v_native.NativeFlow(64, EMB, HID, DEPTH, NFL, activation=act, skip_actnorm=skip_an, skip_shuffle=skip_sh, use_graph=use_graph)
    h.load(sd)
    monkeypatch.delenv(var)
    return h


def _ref64(sd64, x, e, skip_an, skip_sh, act, reverse):
    """float64, composed here from the oracle's leaf functions in the order the flags select (flow_blocks.py:118-136 per block)."""
    from oracle import flow_ref
    h, e = x.double(), e.double()
    logdet = torch.zeros(h.shape[0], dtype=torch.float64)
    for fl in (reversed(range(NFL)) if reverse else range(NFL)):
        p = f"sub_layers.{fl}."
        if not reverse:
            if not skip_an:
                h, ld = flow_ref.actnorm_forward(sd64, p + "norm_layer.", h)
                logdet = logdet + ld
            if act == "lrelu":
                h = flow_ref.inv_lrelu_forward(h)
            h, ld = flow_ref.coupling_forward(sd64, p + "coupling.", h, e, "normal", DEPTH)
            logdet = logdet + ld
            if not skip_sh:
                h = h[:, sd64[p + "shuffle.forward_shuffle_idx"]]
        else:
            if not skip_sh:
                h = h[:, sd64[p + "shuffle.backward_shuffle_idx"]]
            h = flow_ref.coupling_reverse(sd64, p + "coupling.", h, e, "normal", DEPTH)
            if act == "lrelu":
                h = flow_ref.inv_lrelu_reverse(h)
            if not skip_an:
                h = flow_ref.actnorm_reverse(sd64, p + "norm_layer.", h)
    return h, logdet


def test_every_flag_combination_on_every_chain(monkeypatch):
    """8 switch combinations x {folded tile, unfolded tile, generic} chain x B in {3, 17} (one ragged sample tile / two), forward with
    log-det and inverse, against float64; the folded and the unfolded chain give the same bits."""
    sd = T(synth.flow_state_dict(seed=5, n_flows=NFL, embedding_dim=EMB, hidden_dim=HID, hidden_depth=DEPTH))
    sd64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in sd.items()}
    _, residual, embed = synth.bench_inputs(17, 64, EMB)
    for skip_an, skip_sh, act in FLAGS:
        refs = {B: (_ref64(sd64, residual[:B], embed[:B], skip_an, skip_sh, act, False), _ref64(sd64, residual[:B], embed[:B], skip_an, skip_sh, act, True)[0])
                for B in (3, 17)}
        outs = {}
        for chain in CHAINS:
            h = _handle(monkeypatch, chain, sd, skip_an, skip_sh, act)
            for B in (3, 17):
                x, e = residual[:B].cuda().contiguous(), embed[:B].cuda().contiguous()
                zt, ld = h.forward(x, e)
                z = h.inverse(x, e)
                (ztr, ldr), zr = refs[B]
                tag = (skip_an, skip_sh, act, chain, B)
                ez, ezt = rel_l2(z.cpu(), zr), rel_l2(zt.cpu(), ztr)
                print(tag, "rel_l2 inverse %.2e forward %.2e logdet max abs %.2e" % (ez, ezt, float((ld.cpu().double() - ldr).abs().max())))
                assert ezt < TOL and ez < TOL, tag
                assert np.allclose(ld.cpu().numpy(), ldr.numpy(), rtol=1e-4, atol=1e-4), tag
                outs[chain, B] = (zt, ld, z)
        for B in (3, 17):
            for a, b in zip(outs["folded", B], outs["unfolded", B]):
                assert torch.equal(a, b), (skip_an, skip_sh, act, B)


@pytest.mark.parametrize("chain", ["folded", "generic"])
def test_graph_cache_recaptures_and_matches_eager(monkeypatch, chain):
    """use_graph = True against use_graph = False, bit for bit: B = 17, 3, 17 on one handle (each change of B re-captures), then a
    second workspace (re-captures again), both directions; a load() in between drops the cached graphs, so the replay follows the new
    weights."""
    import i2v_native
    sds = [T(synth.flow_state_dict(seed=s, n_flows=NFL, embedding_dim=EMB, hidden_dim=HID, hidden_depth=DEPTH)) for s in (5, 6)]
    _, residual, embed = synth.bench_inputs(17, 64, EMB)
    eager = _handle(monkeypatch, chain, sds[0], use_graph=False)
    graph = _handle(monkeypatch, chain, sds[0], use_graph=True)

    def same(B):
        x, e = residual[:B].cuda().contiguous(), embed[:B].cuda().contiguous()
        zt, ld = eager.forward(x, e)
        z = eager.inverse(x, e)
        for _ in range(2):   # capture, then replay
            gzt, gld = graph.forward(x, e)
            assert torch.equal(gzt, zt) and torch.equal(gld, ld) and torch.equal(graph.inverse(x, e), z), (chain, B)
        return z

    z17 = same(17)
    same(3)
    assert torch.equal(same(17), z17)
    first_ws = graph._ws            # keep the first workspace alive: the second one gets another address
    graph._ws = i2v_native._Workspace()
    same(17)
    assert graph._ws.buf.data_ptr() != first_ws.buf.data_ptr()
    for h in (eager, graph):
        h.load(sds[1])
    assert not torch.equal(same(17), z17)
