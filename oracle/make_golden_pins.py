"""TEST INFRASTRUCTURE -- freezes what tests/test_oracle_pinned.py compares the oracle against, by running the REAL reference.

Run where the reference tree is available (oracle/refshim.py):   python -m oracle.make_golden_pins

Writes, under tests/golden/pins/:
  ops.npz          the index / mask / table generators of models/common/ops.py on the geometries the tests use
                   (masks of 0 / -100 stored as bits)
  net_<case>.npz   whole-network output and a fixed sample (sample_index) of the outputs of the window attention, the
                   anchored-stripe attention and the CAB of layers[0].blocks[2] (window shift + stripe shift active), for the
                   seeded, perturbed weights ``perturb_state_dict(<constructor weights under torch.manual_seed(0)>, 0)``; the
                   tests rebuild those modules' inputs with the oracle (block2_inputs), which is checked here to match the
                   reference's (``oracle_module_inputs_vs_reference_maxabs``)
  grads.npz        a fixed sample of every parameter gradient of more than 4096 elements of oracle/make_golden_grads.py's
                   training-step case; the loss, input gradient, gradient norms and smaller gradients of that case are in
                   tests/golden_grads/, checked here against a fresh reference run (input gradient bitwise, the rest within 1e-6 relative)
The tests rebuild weights and inputs from their seeds and the product constructor, which draws the same initial weights as
the reference (checked here), so the reference tree is needed only to regenerate these files.
"""
import json
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from grl_image_restoration_amd import GRL  # noqa: E402
from grl_image_restoration_amd.presets import make_config  # noqa: E402
from oracle import grl_oracle as O  # noqa: E402
from oracle import make_golden_grads as G  # noqa: E402
from oracle import refshim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pins")

TABLE_CASES = [((4, 86), 1), ((4, 86), 2), ((8, 8), 1), ((8, 8), 2)]
MASK_CASES = [((32, 32), (8, 8), (4, 4), 1), ((16, 64), (8, 32), (4, 16), 4), ((64, 64), (64, 64), (32, 32), 2),
              ((24, 48), (12, 24), (6, 12), 4), ((32, 32), (8, 32), (4, 0), 4)]
NET_CASES = [("tiny", "sr_ckpt_df4", 2, 64), ("base", "yaml", 4, 32)]
MODULE_SAMPLE = 8192      # elements per module output
GRAD_SAMPLE = 2048        # elements per parameter gradient with more than 4096


def tag(*parts):
    return "_".join("x".join(str(v) for v in p) if isinstance(p, (tuple, list)) else str(p) for p in parts)


def pack_mask(m):
    assert m.dtype == torch.float32 and bool(((m == 0) | (m == -100)).all())
    return np.packbits((m == -100).numpy().reshape(-1)), np.array(m.shape, dtype=np.int64)


def unpack_mask(bits, shape):
    n = int(np.prod(shape))
    return torch.from_numpy(np.unpackbits(bits, count=n).reshape(tuple(int(s) for s in shape)).astype(np.float32) * -100.0)


def net_case_weights(cfg):
    torch.manual_seed(0)
    return O.perturb_state_dict(GRL(**cfg).state_dict(), 0)


def make_ops():
    ops = refshim.import_reference_ops()
    arrays = {}
    for win, df in TABLE_CASES:
        arrays["table_" + tag(win, df)] = ops.get_relative_coords_table_all(list(win), [0, 0], df).numpy()
        for w2a in (True, False):
            arrays["index_simple_" + tag(win, df, int(w2a))] = ops.get_relative_position_index_simple(list(win), df, w2a).numpy().astype(np.int32)
            arrays["index_all_" + tag(win, df, int(w2a))] = ops.get_relative_position_index_all(list(win), df, w2a).float().numpy()
    for res, win, shift, df in MASK_CASES:
        t = tag(res, win, shift, df)
        if df == 1:
            arrays["mask_" + t], arrays["mask_shape_" + t] = pack_mask(ops.calculate_mask(list(res), list(win), list(shift)))
        for w2a in (True, False):
            m = ops.calculate_mask_all(list(res), list(win), list(shift), df, w2a)
            arrays["mask_all_" + t + f"_{int(w2a)}"], arrays["mask_all_shape_" + t + f"_{int(w2a)}"] = pack_mask(m)
    np.savez_compressed(os.path.join(OUT, "ops.npz"), **arrays)
    print(f"ops: {len(arrays)} arrays")


def sample_index(n, k, seed):
    """A fixed sample of k of n flat positions (numpy's legacy RandomState: its stream is frozen across versions)."""
    return np.unique(np.random.RandomState(seed).randint(0, n, size=min(k, n)))


def block2_inputs(cfg, sd, lq, x_size):
    """The oracle's output and the inputs of the window attention, the anchored-stripe attention and the CAB of
    layers[0].blocks[2], computed from block 1's output the way mixed_attention / block_forward do."""
    import torch.nn.functional as F

    cap = {}
    with torch.no_grad():
        y = O.grl_forward(lq, cfg, sd, capture=cap)
        x = cap["layers.0.blocks.1"]
        pre = "layers.0.blocks.2.attn."
        qkv = F.linear(x, sd[pre + "qkv.body.weight"], sd[pre + "qkv.body.bias"])
        qkv_w, qkv_s = torch.split(qkv, x.shape[-1] * 3 // 2, dim=-1)
        anchor = O.anchor_projection(x, x_size, O.block_schedule(cfg, x_size)[0][2]["df"], sd, pre + "anchor.")
    ins = dict(win_qkv=qkv_w.contiguous(), stripe_qkv=qkv_s.contiguous(), stripe_anchor=anchor)
    if cfg["local_connection"]:
        ins["cab_x"] = x
    return y, ins


def make_net(model, geom, up, size):
    GRL_ref = refshim.import_reference_grl()
    cfg = make_config(model, geom, upscale=up, img_size=size)
    torch.manual_seed(0)
    ref = GRL_ref(**cfg).eval()
    sd = O.perturb_state_dict(ref.state_dict(), 0)
    mine = net_case_weights(cfg)
    assert all(torch.equal(mine[k], sd[k]) for k in mine), "product constructor no longer draws the reference's initial weights"
    ref.load_state_dict(sd)
    lq, _ = O.synthetic_pair("sr", (size, size), up)
    cap = {}
    blk = ref.layers[0].blocks[2]
    hooks = [blk.attn.window_attn.register_forward_hook(lambda m, i, o: cap.__setitem__("win", (i, o))),
             blk.attn.stripe_attn.register_forward_hook(lambda m, i, o: cap.__setitem__("stripe", (i, o)))]
    if cfg["local_connection"]:
        hooks.append(blk.conv.register_forward_hook(lambda m, i, o: cap.__setitem__("cab", (i, o))))
    with torch.no_grad():
        y = ref(lq)
    for h in hooks:
        h.remove()
    (qkv_w, x_size, *_), win_out = cap["win"]
    (qkv_s, anchor, *_), stripe_out = cap["stripe"]
    ref_ins = dict(win_qkv=qkv_w, stripe_qkv=qkv_s, stripe_anchor=anchor)
    outs = dict(win_out=win_out, stripe_out=stripe_out)
    if cfg["local_connection"]:
        (cab_x, _), outs["cab_out"] = cap["cab"]
        ref_ins["cab_x"] = cab_x
    x_size = tuple(int(v) for v in x_size)
    yo, ins = block2_inputs(cfg, mine, lq, x_size)
    assert set(ins) == set(ref_ins)
    in_err = max(float((ins[k] - ref_ins[k]).abs().max()) for k in ins)
    # the module outputs are stored as a fixed sample (the whole tensors would not be small test vectors)
    arrays = dict(output=y.numpy())
    for k, v in outs.items():
        arrays[k + "_sample"] = v.reshape(-1).numpy()[sample_index(v.numel(), MODULE_SAMPLE, zlib.crc32(k.encode()))]
    meta = dict(cfg=cfg, x_size=list(x_size), module_sample=MODULE_SAMPLE, oracle_vs_reference_maxabs=float((y - yo).abs().max()),
                oracle_module_inputs_vs_reference_maxabs=in_err)
    name = "net_" + tag(model, geom, up, size)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), meta=json.dumps(meta), **arrays)
    print(f"{name}: oracle-vs-reference max|d| = {meta['oracle_vs_reference_maxabs']:.3e}, module inputs {in_err:.3e}")


def grads_case_weights(cfg):
    shapes = {k: tuple(v.shape) for k, v in GRL(**cfg).state_dict().items()}
    return O.seeded_state_dict(shapes, seed=0)


def make_grads():
    """Samples of the gradients the tracked fixture tests/golden_grads/train_base2x2_sr4_64.npz holds only as norms; its loss,
    input gradient, norms and small tensors are checked here against a fresh reference run (input gradient bitwise, the rest within 1e-6 relative)."""
    cfg, sd, lq, gt = G.make_case()
    mine = grads_case_weights(cfg)
    assert set(mine) == {k for k in sd if not k.startswith(("table_", "index_", "mask_"))}
    assert all(torch.equal(mine[k], sd[k]) for k in mine)
    loss, gin, grads = G.reference_step(cfg, sd, lq, gt)
    z = np.load(os.path.join(ROOT, "tests", "golden_grads", G.NAME + ".npz"), allow_pickle=False)
    zmeta = json.loads(str(z["meta"]))
    assert zmeta["cfg"] == json.loads(json.dumps(cfg)) and zmeta["loss"] == float(loss)
    assert np.array_equal(z["input"], lq.numpy()) and np.array_equal(z["target"], gt.numpy()) and np.array_equal(z["grad_input"], gin.numpy())
    names = sorted(grads)
    assert json.loads(str(z["grad_norm_names"])) == names
    # (the reference's own CPU reductions move norms and small gradients by ~1e-7 relative from run to run)
    norms = np.array([grads[k].norm().item() for k in names], dtype=np.float64)
    drift = float(np.max(np.abs(norms - z["grad_norms"]) / z["grad_norms"]))
    arrays = {}
    for k in names:
        g = grads[k]
        if g.numel() <= 4096:
            r = z["grad::" + k]
            drift = max(drift, float(np.linalg.norm(r - g.numpy()) / max(np.linalg.norm(r), 1e-30)))
        else:
            arrays["sample::" + k] = g.reshape(-1).numpy()[sample_index(g.numel(), GRAD_SAMPLE, zlib.crc32(k.encode()))]
    assert drift < 1e-6, drift
    np.savez_compressed(os.path.join(OUT, "grads.npz"), meta=json.dumps(dict(grad_sample=GRAD_SAMPLE, tracked_fixture_max_rel_drift=drift)), **arrays)
    print(f"grads: loss {float(loss):.6f}, {len(grads)} parameter gradients, {len(arrays)} sampled, tracked fixture within {drift:.2e}")


def main():
    os.makedirs(OUT, exist_ok=True)
    make_ops()
    for case in NET_CASES:
        make_net(*case)
    make_grads()


if __name__ == "__main__":
    main()
