#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ by running THE REFERENCE ITSELF.

Runs only in the build container, where the reference checkout is mounted read-only at
/root/reference.  It imports the reference's ``Generator`` (model.py:15), loads the
deterministic synthetic weights of ``mocha_sigasia2023_amd.weights`` into it with
``load_state_dict(strict=True)`` (which also pins the key schema and, through the buffer
comparison below, the regenerated graph constants), runs the demo's call sequence
(test_fullframework.py:190-193,301-302) and ``Generator.forward`` (model.py:82-106) on
seeded synthetic windows, and stores inputs + outputs as ``.npz``.  The matching fixture
runs scikit-learn's ``BallTree`` exactly as the demo does (test_fullframework.py:294-296).

No reference source or bytecode is written anywhere; the fixtures are data only.

    python tests/golden/make_golden.py            # regenerates every fixture
"""
import os
import sys
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("MOCHA_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

from mocha_sigasia2023_amd import synthetic, weights  # noqa: E402
from mocha_sigasia2023_amd.skeleton import skeleton_constants  # noqa: E402


def build_reference_generator(layout, overrides=None):
    """Instantiate the reference Generator; for 'mixamo' swap the two hard-coded 'mocha'
    pool modules after construction."""
    cwd = os.getcwd()
    os.chdir(REF)  # model.py:7-8 appends './net', './motion' relative to cwd
    try:
        for p in (REF, os.path.join(REF, "net"), os.path.join(REF, "etc")):
            if p not in sys.path:
                sys.path.append(p)
        from utils import get_config          # etc/utils.py:23-25
        from model import Generator           # model.py:15
        from graph import PoolJointToBodypart, UnpoolBodypartToJoint
        from transformer import mean_variance_norm
        cfg = get_config(os.path.join(REF, "configs/config.yaml"))["model"]
        if layout != "mocha":
            cfg["graph"]["joint"]["layout"] = layout
            cfg["graph"]["bodypart"]["layout"] = layout
        for k, v in (overrides or {}).items():              # configs/config.yaml:13-31: depths, heads, head dims
            assert k in cfg, k
            cfg[k] = v
        G = Generator(cfg)
        if layout != "mocha":
            G.mot_embedding[3] = PoolJointToBodypart(layout)
            G.to_mot[3] = UnpoolBodypartToJoint(layout)
    finally:
        os.chdir(cwd)
    return G.eval(), mean_variance_norm


def run_variant(name, layout, seed, gain, B):
    G, mvn = build_reference_generator(layout)
    ref_buffers = {k: v.numpy().copy() for k, v in G.state_dict().items()
                   if k.endswith("A_j") or k.endswith("A_b") or k in ("mot_embedding.3.weight", "to_mot.3.weight")}
    sd = weights.synthetic_state_dict(seed=seed, gain=gain, layout=layout)
    # a14: our regenerated graph constants must equal the reference's own buffers bit for bit
    for k, v in ref_buffers.items():
        assert v.shape == sd[k].shape and np.array_equal(v, sd[k]), f"graph constant mismatch: {k}"
    G.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    V = skeleton_constants(layout).V
    src = torch.from_numpy(synthetic.pose_windows(seed + 1, B, V))
    cha = torch.from_numpy(synthetic.pose_windows(seed + 2, B, V))
    out = {"src_X": src.numpy(), "cha_X": cha.numpy()}
    with torch.no_grad():
        # the demo's sequence, test_fullframework.py:190-193
        for tag, X in (("src", src), ("cha", cha)):
            tokens = G.mot_embedding(X)
            out[f"{tag}_tokens"] = tokens.numpy()
            tokens = tokens + G.pos_emb[:, :tokens.shape[1]]
            encoded = G.encoder(tokens)
            out[f"{tag}_encoded"] = encoded.numpy()
            cnt = mvn(encoded.permute(0, 2, 1)).permute(0, 2, 1)
            out[f"{tag}_cnt"] = cnt.numpy()
        # sub-stage taps (module boundaries of model.py:42-50 and :71-80)
        x = G.mot_embedding[:5](src)                       # after AvgPool2d: (B, 256, 15, 6)
        out["src_emb_pooled"] = x.numpy()
        enc_s = torch.from_numpy(out["src_encoded"])
        enc_c = torch.from_numpy(out["cha_encoded"])
        dec = G.decoder(enc_s, enc_c)                      # test_fullframework.py:301
        out["decoded"] = dec.numpy()
        out["mot_body"] = G.to_mot[:2](dec).numpy()        # after the body block: (B, 256, 15, 6)
        Y = G.to_mot(dec)                                  # :302
        out["Y"] = Y.numpy()
        Yf = G(src, cha)                                   # model.py:82-106
        assert torch.equal(Yf, Y) or float((Yf - Y).abs().max()) < 1e-6
        out["Y_forward"] = Yf.numpy()
    meta = dict(layout=layout, seed=seed, gain=gain, B=B, V=V,
                torch=torch.__version__, numpy=np.__version__)
    path = os.path.join(HERE, f"generator_{name}.npz")
    np.savez(path, **out, meta=np.array(repr(meta)))
    print(name, {k: (v.shape, float(np.abs(v).max())) for k, v in out.items()})
    return path


# model configurations other than the shipped one (model.py:16-80 reads them from the config): the reference built with them, our
# seeded weights of those shapes, B = 2; only the outputs are stored (inputs and weights are regenerated from the seeds)
CONFIG_VARIANTS = {
    "e1h4d128_d3h4d256": dict(encoder_depth=1, decoder_depth=3),
    "e2h4d256_d2h4d128": dict(encoder_dim_head=256, decoder_dim_head=128),
    "e3h8d128_d1h2d256": dict(encoder_depth=3, encoder_heads=8, decoder_depth=1, decoder_heads=2),
    "e2h1d128_d4h3d256": dict(encoder_heads=1, decoder_depth=4, decoder_heads=3),
    # the reference Attention's own default head dim (net/transformer.py:38) and other feed-forward widths (model.py:18-33 reads them from YAML)
    "e2h4d64_d2h8d64_mlp256_1024": dict(encoder_dim_head=64, decoder_heads=8, decoder_dim_head=64, encoder_mlp_dim=256, decoder_mlp_dim=1024),
    "e2h4d128_d2h4d256_mlp768_320": dict(encoder_mlp_dim=768, decoder_mlp_dim=320),
}


def run_config_variants():
    out = {}
    for name, ov in CONFIG_VARIANTS.items():
        G, mvn = build_reference_generator("mocha", ov)
        cfg = dict(weights.DEFAULT_CFG, **ov)
        sd = weights.synthetic_state_dict(seed=909, gain=1.3, layout="mocha", cfg=cfg)
        G.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        src = torch.from_numpy(synthetic.pose_windows(910, 2, 24)); cha = torch.from_numpy(synthetic.pose_windows(911, 2, 24))
        with torch.no_grad():
            tokens = G.mot_embedding(cha)
            enc = G.encoder(tokens + G.pos_emb[:, :tokens.shape[1]])
            out[f"{name}_cha_encoded"] = enc.numpy()
            out[f"{name}_Y_forward"] = G(src, cha).numpy()
    np.savez(os.path.join(HERE, "generator_config_variants.npz"), **out,
             meta=np.array(repr(dict(seed=909, gain=1.3, src_seed=910, cha_seed=911, B=2, variants=CONFIG_VARIANTS, torch=torch.__version__))))
    print("config variants", {k: (v.shape, float(np.abs(v).max())) for k, v in out.items()})


def run_graph_constants():
    """Reference buffers for both layouts (row a14), stored so the CPU test needs no reference."""
    out = {}
    for layout in ("mocha", "mixamo"):
        G, _ = build_reference_generator(layout)
        sd = G.state_dict()
        out[f"{layout}_A_j"] = sd["mot_embedding.2.A_j"].numpy()
        out[f"{layout}_A_b"] = sd["mot_embedding.5.A_b"].numpy()
        out[f"{layout}_pool"] = sd["mot_embedding.3.weight"].numpy()
        out[f"{layout}_unpool"] = sd["to_mot.3.weight"].numpy()
    np.savez(os.path.join(HERE, "graph_constants.npz"), **out)


def run_match():
    """BallTree k=1 exactly as test_fullframework.py:293-296,440-443, on seeded synthetic cnt."""
    import sklearn
    from sklearn.neighbors import BallTree
    out = {}
    mean, std = synthetic.cnt_norm(90)
    for nb, q, seed in ((64, 16, 100), (585, 16, 200)):
        cha_cnt = synthetic.token_features(seed, nb)
        src_cnt = synthetic.token_features(seed + 1, q)
        # make a few queries near-duplicates of bank rows so the answer is not arbitrary
        src_cnt[:4] = cha_cnt[[3, nb - 1, nb // 2, 7]] + 0.05 * src_cnt[:4]
        cha_nm = (cha_cnt - mean[np.newaxis]) / std[np.newaxis]
        tree = BallTree(cha_nm.reshape(cha_nm.shape[0], -1))
        src_nm = (src_cnt - mean[np.newaxis]) / std[np.newaxis]
        dist, idx = tree.query(src_nm.reshape(src_nm.shape[0], -1), k=1, return_distance=True)
        out[f"n{nb}_idx"] = idx[:, 0].astype(np.int64)
        out[f"n{nb}_dist"] = dist[:, 0].astype(np.float64)
        out[f"n{nb}_seed"] = np.array([seed, nb, q])
    out["meta"] = np.array(repr(dict(sklearn=sklearn.__version__, cnt_norm_seed=90)))
    np.savez(os.path.join(HERE, "match_balltree.npz"), **out)
    print("match", {k: v for k, v in out.items() if k.endswith("idx")})


CVAE_ARITHMETIC = {"MKL_CBWR": "COMPATIBLE", "ATEN_CPU_CAPABILITY": "default", "OMP_NUM_THREADS": "1", "MKL_NUM_THREADS": "1"}


def run_cvae():
    """CVAE.sample(c, deterministic=True) of the reference (model_CVAE.py:44-46) with synthetic weights,
    constructed as the demo does (test_fullframework.py:52-58).  Recorded on the arithmetic tests/test_cvae_oracle.py
    re-runs the oracle on: MKL's reproducible COMPATIBLE path, ATen's non-vectorised kernels, one thread - the same bits
    on any x86-64 CPU, where the default dispatch picks AVX2 or AVX-512 code by CPU and moves `out` by up to 1e-5.  Both
    libraries read these settings when they load, so they are set in the environment of the whole run:
        env MKL_CBWR=COMPATIBLE ATEN_CPU_CAPABILITY=default OMP_NUM_THREADS=1 MKL_NUM_THREADS=1 python tests/golden/make_golden.py run_cvae"""
    unset = {k: v for k, v in CVAE_ARITHMETIC.items() if os.environ.get(k) != v}
    if unset:
        raise SystemExit(f"run_cvae: set {unset} in the environment (see the docstring)")
    torch.set_num_threads(1)
    cwd = os.getcwd(); os.chdir(REF)
    try:
        if REF not in sys.path:
            sys.path.append(REF)
        import torch.nn.functional as F
        from model_CVAE import CVAE
        net = CVAE(output_seq=90, latent_dim=256, depth=2, nheads=4, feedforward_dim=512, dropout=0.1, activation=F.relu).eval()
    finally:
        os.chdir(cwd)
    sd = weights.synthetic_cvae_state_dict(seed=99, gain=1.0)
    ref_sd = net.state_dict()
    for k, v in sd.items():
        assert tuple(ref_sd[k].shape) == v.shape, k
    missing, unexpected = net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith("encoder.") or k.endswith("pos_encoder.pe") for k in missing), missing
    assert np.array_equal(ref_sd["prior_net.pos_encoder.pe"][0, :182].numpy(), weights.sincos_pe(182))
    c = torch.from_numpy(synthetic.token_features(500, 2 * 2).reshape(2, 180, 256))
    with torch.no_grad():
        mu, logvar = net.prior(c)
        out = net.sample(c, deterministic=True)
    np.savez(os.path.join(HERE, "cvae_sample.npz"), c=c.numpy(), mu=mu.numpy(), logvar=logvar.numpy(), out=out.numpy(),
             meta=np.array(repr(dict(seed=99, gain=1.0, torch=torch.__version__, arithmetic=CVAE_ARITHMETIC))))
    print("cvae", {k: float(np.abs(v).max()) for k, v in dict(mu=mu.numpy(), logvar=logvar.numpy(), out=out.numpy()).items()})


def run_featurize(layout="mocha", seed=321, name="featurize.npz"):
    """test_fullframework.py:141-185 executed with the reference's own quaternion library (motion/quat.py)
    on synthetic local bone features; only the X features are stored."""
    sys.path.insert(0, os.path.join(REF, "motion"))
    import quat                                           # the reference's motion/quat.py
    from mocha_sigasia2023_amd.skeleton import LAYOUTS
    parents = np.concatenate([[-1], np.asarray(LAYOUTS[layout]["parents"]) + 1])   # :101-102
    window = 60
    Yrot, Ypos, Yvel, Yang = synthetic.bone_windows(seed, 3, J=len(parents))
    Grot, Gpos, Gvel, Gang = quat.fk_vel(Yrot, Ypos, Yvel, Yang, parents)
    Gpos[:, :, 0:1] = np.repeat(Gpos[:, -1:, 0:1], window, axis=1)
    Grot[:, :, 0:1] = np.repeat(Grot[:, -1:, 0:1], window, axis=1)
    Gvel[:, :, 0:1] = np.repeat(Gvel[:, -1:, 0:1], window, axis=1)
    Gang[:, :, 0:1] = np.repeat(Gang[:, -1:, 0:1], window, axis=1)
    Xpos = quat.inv_mul_vec(Grot[:, :, 0:1], Gpos - Gpos[:, :, 0:1])
    Xrot = quat.inv_mul(Grot[:, :, 0:1], Grot)
    Xtxy = quat.to_xform_xy(Xrot).astype(np.float32)
    Xvel = quat.inv_mul_vec(Grot[:, :, 0:1], Gvel)
    Xang = quat.inv_mul_vec(Grot[:, :, 0:1], Gang)
    b, ns, nj, _, _ = Xtxy.shape
    X = np.concatenate([Xpos, Xtxy.reshape(b, ns, nj, -1), Xvel, Xang], axis=-1)
    np.savez(os.path.join(HERE, name), X=X.astype(np.float32), seed=np.array([seed, 3]))
    print(name, X.shape, X.dtype, float(np.abs(X).max()))


def run_featurize_mixamo():
    """The second layout (23 bones): the one live sessions run on."""
    run_featurize("mixamo", 322, "featurize_mixamo.npz")


def run_database():
    """Row N4's tail: a small synthetic ``database.bin`` in the byte layout preprocess/generate_database_bin.py:228-246 writes,
    read back with THE REFERENCE's ``load_database`` (etc/utils.py:144-190); the step-1 windowing, FK / re-rooting and z-score
    by EXECUTING lines 93-165 of the reference's collect_CVAE_feature_action.py (its ``main`` is not importable piecewise) in a
    namespace prepared with that file's own variable names.  Stored: the file bytes, what the reference reader returns, the
    reference's window ranges / labels / first frames, and its normalised features X for a few windows."""
    import io
    import struct
    import textwrap
    sys.path.insert(0, os.path.join(REF, "motion")); sys.path.insert(0, os.path.join(REF, "etc"))
    import quat
    from utils import load_database as ref_load_database
    from mocha_sigasia2023_amd.skeleton import LAYOUTS
    r = np.random.Generator(np.random.PCG64(2024))
    lengths, styles, actions = [75, 64, 90, 61, 70], [2, 2, 5, 2, 2], [1, 3, 1, 4, 2]
    nframes, nbones = sum(lengths), 25
    rot = r.standard_normal((nframes, nbones, 4)).astype(np.float32)
    rot /= np.sqrt((rot * rot).sum(-1, keepdims=True)); rot = np.where(rot[..., :1] > 0, rot, -rot).astype(np.float32)
    db = {"bone_positions": (0.3 * r.standard_normal((nframes, nbones, 3))).astype(np.float32),
          "bone_velocities": r.standard_normal((nframes, nbones, 3)).astype(np.float32), "bone_rotations": rot,
          "bone_angular_velocities": r.standard_normal((nframes, nbones, 3)).astype(np.float32),
          "bone_parents": np.concatenate([[-1], np.asarray(LAYOUTS["mocha"]["parents"]) + 1]).astype(np.int32),
          "range_starts": np.cumsum([0] + lengths[:-1]).astype(np.int32), "range_stops": np.cumsum(lengths).astype(np.int32),
          "style_labels": np.asarray(styles, np.int32), "action_labels": np.asarray(actions, np.int32),
          "contact_states": (r.uniform(size=(nframes, 2)) > 0.5).astype(np.uint8)}
    buf = io.BytesIO()                                    # preprocess/generate_database_bin.py:235-246, same order and headers
    for k in ("bone_positions", "bone_velocities", "bone_rotations", "bone_angular_velocities"):
        buf.write(struct.pack("II", nframes, nbones) + db[k].ravel().tobytes())
    buf.write(struct.pack("I", nbones) + db["bone_parents"].ravel().tobytes())
    for k in ("range_starts", "range_stops", "style_labels", "action_labels"):
        buf.write(struct.pack("I", len(lengths)) + db[k].ravel().tobytes())
    buf.write(struct.pack("II", nframes, 2) + db["contact_states"].ravel().tobytes())
    raw = buf.getvalue()
    tmp = os.path.join("/tmp", "mocha_golden_database.bin")
    open(tmp, "wb").write(raw)
    database = ref_load_database(tmp)                     # the reference reader
    out = {"bin": np.frombuffer(raw, dtype=np.uint8)}
    import hashlib
    for k, v in database.items():                         # what the reference reader returned: small arrays verbatim, the frame arrays
        v = np.asarray(v)                                 # (already in `bin`) as shape + dtype + SHA-256 of their bytes
        if v.size <= 64:
            out["db_" + k] = v
        else:
            out["dbsha_" + k] = np.array([str(v.shape), str(v.dtype), hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()])
    # ---- the reference's windowing + featurisation, executed from its own source text
    src = open(os.path.join(REF, "collect_CVAE_feature_action.py")).read().splitlines()
    code = textwrap.dedent("\n".join(src[92:165]))        # lines 93-165
    Xm = r.standard_normal((1, 1, 25, 15)).astype(np.float32); Xs = r.uniform(0.5, 2.0, (1, 1, 25, 15)).astype(np.float32)
    ns = {"np": np, "quat": quat, "parents": database["bone_parents"], "contacts": database["contact_states"],
          "range_starts": database["range_starts"], "range_stops": database["range_stops"], "style_labels": database["style_labels"],
          "action_labels": database["content_labels"],    # the reader's name for them (etc/utils.py:172-173)
          "Ypos": database["bone_positions"].astype(np.float32), "Yrot": database["bone_rotations"].astype(np.float32),
          "Yvel": database["bone_velocities"].astype(np.float32), "Yang": database["bone_angular_velocities"].astype(np.float32),
          "target_style_label": [2], "target_action_label": [1, 3, 4], "style_names": ["s%d" % i for i in range(8)],
          "action_names": ["a%d" % i for i in range(8)], "X_mean": Xm, "X_std": Xs, "print": lambda *a, **k: None}
    exec(compile(code, "collect_CVAE_feature_action.py[93:165]", "exec"), ns)
    N = len(ns["action_label"])
    # first frame of every window: located by matching the reference's slices in the frame arrays
    pos = database["bone_positions"]
    starts = np.array([next(g for g in range(nframes - 59) if np.array_equal(pos[g:g + 60], ns["Ypos"][k])) for k in range(N)], np.int64)
    sel = np.array([0, 7, N // 2, N - 1])
    out.update(range_starts=ns["cha_range_starts"], range_stops=ns["cha_range_stops"], action_label=ns["action_label"], starts=starts,
               X_sel=ns["X"][sel].astype(np.float32), sel=sel, X_mean=Xm, X_std=Xs, style_keep=np.array([2]), action_keep=np.array([1, 3, 4]))
    np.savez_compressed(os.path.join(HERE, "database_bank.npz"), **out)
    os.remove(tmp)
    print("database", {k: getattr(v, "shape", v) for k, v in out.items() if not k.startswith("db_")})


def run_postprocess(layout="mocha", contact_bones=(5, 24), seed=77, cm_seed=78, name="postprocess.npz"):
    """The demo's per-frame post-processing, produced by EXECUTING THE REFERENCE'S OWN LINES: test_fullframework.py:289-641 (the body
    of its `with torch.no_grad():` block - frame 0 at :289-437, the frame loop at :438-641) and :643-694 (stacking, root merge),
    taken from its source text and run in a prepared namespace, as run_database does for collect_CVAE_feature_action.py.
    Nothing of the loop is re-written here: the namespace only supplies what the script computed earlier in main() -
    stand-ins for the network (model.decoder / model.to_mot hand out the seeded synthetic decoded windows, CVAE branch and NN
    branch separately; network_cvae.sample returns its input's second half), the source clip's arrays, constants - and the
    reference's quat / Inertialization modules.  Both branches are stored: "Ours" (blend + foot-lock IK, :529-631) and the
    context-matching "cm_" branch (no blend, no IK, :512-527, 637-641)."""
    cwd = os.getcwd(); os.chdir(REF)
    try:
        sys.path.insert(0, os.path.join(REF, "motion"))
        import quat
        import Inertialization as inert
    finally:
        os.chdir(cwd)
    from sklearn.neighbors import BallTree
    from mocha_sigasia2023_amd.skeleton import LAYOUTS
    N = 120
    par0 = np.asarray(LAYOUTS[layout]["parents"])
    J = len(par0) + 1
    Y, rvel, rang, hipvel, contact = synthetic.postprocess_inputs(seed, N, V=J - 1)   # "Ours" branch windows + the source's signals
    Ycm = synthetic.postprocess_inputs(cm_seed, N, V=J - 1)[0]                        # NN ("cm_") branch windows
    r = np.random.Generator(np.random.PCG64(123))

    class _Tokens:                                        # what model.decoder returns: which window to_mot must hand out
        def __init__(self, frame, branch): self.frame, self.branch = frame, branch

    class _Model:
        """decoder is called twice per frame, CVAE branch first, NN branch second (test_fullframework.py:301,311 / 455,465)."""
        calls = 0
        def decoder(self, src, cha):
            t = _Tokens(self.calls // 2, self.calls % 2); self.calls += 1
            return t
        def to_mot(self, t):
            return torch.from_numpy((Ycm if t.branch else Y)[t.frame][None])

    class _CVAE:
        def sample(self, condition, deterministic=False):
            return condition[:, condition.shape[1] // 2:]

    src_Yrvel = r.standard_normal((N, 60, 3)).astype(np.float32); src_Yrvel[:, -1] = rvel
    src_Yrang = r.standard_normal((N, 60, 3)).astype(np.float32); src_Yrang[:, -1] = rang
    src_Yvel = r.standard_normal((N, 60, J, 3)).astype(np.float32); src_Yvel[:, :, 1] = hipvel
    src_contact = (r.uniform(size=(N, 60, 2)) > 0.5).astype(np.uint8); src_contact[:, -1] = contact
    ns = {
        "np": np, "torch": torch, "quat": quat, "inert": inert, "BallTree": BallTree, "device": torch.device("cpu"),
        "model": _Model(), "network_cvae": _CVAE(),
        # the matching inputs only steer which bank row the NN branch names; the stand-in decoder ignores it
        "src_encoded": torch.zeros((N, 2, 3)), "src_cnt": r.standard_normal((N, 2, 3)).astype(np.float32),
        "cha_cnt": r.standard_normal((7, 2, 3)).astype(np.float32), "cha_encoded": torch.zeros((7, 2, 3)),
        "cnt_mean": np.zeros((2, 3), np.float32), "cnt_std": np.ones((2, 3), np.float32),
        "src_cnt_mean": torch.zeros((2, 3)), "src_cnt_std": torch.ones((2, 3)),
        "cha_encoded_mean": torch.zeros((2, 3)), "cha_encoded_std": torch.ones((2, 3)),
        "Y_mean": np.zeros((1, 1, J, 15), np.float32), "Y_std": np.ones((1, 1, J, 15), np.float32),      # windows are de-normalised already
        "src_Ypos": r.standard_normal((N, 60, J, 3)).astype(np.float32), "src_Yvel": src_Yvel,
        "src_Yrot": np.tile(np.array([1, 0, 0, 0], np.float32), (N, 60, J, 1)), "src_Yang": r.standard_normal((N, 60, J, 3)).astype(np.float32),
        "src_Yrvel": src_Yrvel, "src_Yrang": src_Yrang, "src_contact": src_contact,
        "parents": np.concatenate([[-1], par0 + 1]), "contact_bones": np.array(contact_bones), "dt": 1.0 / 60.0,
        "ik_enabled": True, "ik_max_length_buffer": 0.015, "ik_foot_height": 0.02, "ik_toe_length": 0.15,
        "ik_unlock_radius": 0.2, "ik_blending_halflife": 0.1,
        "animation_plot": lambda *a, **k: None,
    }
    src = open(os.path.join(REF, "test_fullframework.py")).read().splitlines()
    assert src[287].strip() == "with torch.no_grad():" and src[642].startswith("    src_Ypos = np.stack(src_Ypos_list")
    loop = textwrap.dedent("\n".join(src[288:641]))       # lines 289-641
    with torch.no_grad():
        exec(compile(loop, "test_fullframework.py[289:641]", "exec"), ns)
    pre = {k: np.stack(ns[k + "_list"]) for k in ("trans_Ypos", "trans_Yrot", "ik_trans_Ypos", "ik_trans_Yrot", "cm_trans_Ypos", "cm_trans_Yrot")}
    tail = textwrap.dedent("\n".join(src[642:694]))       # lines 643-694: np.stack of every list, quat.fk, root merge
    exec(compile(tail, "test_fullframework.py[643:694]", "exec"), ns)
    assert ns["model"].calls == 2 * N
    assert np.array_equal(pre["trans_Ypos"], pre["ik_trans_Ypos"])      # IK never moves positions: one list serves both (:627, :633)
    # what the library computes per window before the loop (:457-462 and the ratio's numerator :492): reference functions on the windows
    heads_rot = np.stack([quat.from_xform_xy(Y[i][-1, :, 3:9].reshape(-1, 3, 2)) for i in range(N)])
    speed = np.array([np.linalg.norm(Y[i][..., 9:12][:, 0], axis=1).mean() for i in range(N)], np.float32)
    cm_speed = np.array([np.linalg.norm(Ycm[i][..., 9:12][:, 0], axis=1).mean() for i in range(N)], np.float32)
    np.savez(os.path.join(HERE, name), seed=np.array([seed, N]), cm_seed=np.array([cm_seed, N]),
             pos=pre["ik_trans_Ypos"], rot=pre["trans_Yrot"], ik_rot=pre["ik_trans_Yrot"],
             cm_pos=pre["cm_trans_Ypos"], cm_rot=pre["cm_trans_Yrot"],
             heads_rot=heads_rot.astype(np.float32), speed=speed, cm_speed=cm_speed,
             bvh_pos=ns["ik_trans_Ypos"], bvh_euler=np.degrees(quat.to_euler(ns["ik_trans_Yrot"])),          # :706-707
             cm_bvh_pos=ns["cm_trans_Ypos"], cm_bvh_euler=np.degrees(quat.to_euler(ns["cm_trans_Yrot"])))
    print(name, pre["ik_trans_Ypos"].shape, float(np.abs(pre["ik_trans_Ypos"]).max()), "ik changed rotations on",
          int((np.abs(pre["ik_trans_Yrot"] - pre["trans_Yrot"]).max(axis=(1, 2)) > 1e-9).sum()), "frames")


MIXAMO_POST_SEEDS = (170, 171)          # "Ours" / "cm_" inputs: 170 reaches every contact transition on this skeleton (tests/test_live_oracle.py)


def run_postprocess_mixamo():
    """The second layout: parents of LAYOUTS["mixamo"], the toes (bones 18 and 22 of the 23-bone skeleton) as contact bones."""
    run_postprocess("mixamo", (18, 22), *MIXAMO_POST_SEEDS, name="postprocess_mixamo.npz")


def run_bvh():
    """The reference writer (motion/bvh.py:179-224) on a small seeded animation; the produced text is the expected output."""
    import tempfile
    sys.path.insert(0, os.path.join(REF, "motion"))
    import bvh
    from mocha_sigasia2023_amd.skeleton import LAYOUTS
    parents = np.asarray(LAYOUTS["mocha"]["parents"])
    r = np.random.Generator(np.random.PCG64(5))
    V, N = len(parents), 4
    pos = r.standard_normal((N, V, 3)); rot = 90.0 * r.standard_normal((N, V, 3))
    names = ["Bone%02d" % i for i in range(V)]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "o.bvh")
        bvh.save(path, {"rotations": rot, "positions": pos, "offsets": pos[0], "parents": parents, "names": names, "order": "zyx"})
        text = open(path).read()
    np.savez(os.path.join(HERE, "bvh_writer.npz"), pos=pos, rot=rot, text=np.array(text))
    print("bvh", len(text), "chars")


def run_checkpoint_schema():
    """The checkpoint FILE schema, from the reference's own writer: Trainer(cfg).save_checkpoint (trainer.py:210-222) into a
    temporary directory, read back with torch.load as Trainer.load_checkpoint / the demo do (trainer.py:224-247,
    test_fullframework.py:47-49) -> the top-level keys, and name / shape / dtype of every entry of 'gen' and 'gen_ema', as JSON.
    The CVAE's file is a bare state_dict (test_fullframework.py:52-58): its key list too.  Data only."""
    import json
    import tempfile
    cwd = os.getcwd(); os.chdir(REF)
    try:
        for p in (REF, os.path.join(REF, "net"), os.path.join(REF, "etc"), os.path.join(REF, "motion")):
            if p not in sys.path:
                sys.path.append(p)
        from utils import get_config
        from trainer import Trainer                       # trainer.py:17
        from model_CVAE import CVAE                       # model_CVAE.py
        import torch.nn.functional as F
        cfg = get_config(os.path.join(REF, "configs/config.yaml"))
        with tempfile.TemporaryDirectory() as tmp:
            cfg["model_dir"] = tmp                        # etc/utils.py initialize_path would create it under the reference tree
            tr = Trainer(cfg)
            tr.save_checkpoint(125)
            path = os.path.join(tmp, "gen_125.pt")
            ck = torch.load(path, map_location="cpu")
            wrapped = {"module." + k for k in ck["gen_ema"]} == set(torch.nn.DataParallel(tr.gen_ema.module if hasattr(tr.gen_ema, "module") else tr.gen_ema).state_dict())
        net = CVAE(output_seq=90, latent_dim=256, depth=2, nheads=4, feedforward_dim=512, dropout=0.1, activation=F.relu)   # test_fullframework.py:52-55
    finally:
        os.chdir(cwd)
    desc = lambda sd: {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()}
    out = {"file": "gen_%03d.pt" % 125, "top_level_keys": list(ck.keys()), "gen": desc(ck["gen"]), "gen_ema": desc(ck["gen_ema"]),
           "gen_opt_keys": list(ck["gen_opt"].keys()), "dataparallel_prefix": "module.", "dataparallel_prefix_checked": bool(wrapped),
           "cvae_file": "cvae_020000.pt", "cvae": desc(net.state_dict())}
    with open(os.path.join(HERE, "checkpoint_schema.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"checkpoint_schema.json: {len(out['gen_ema'])} gen_ema entries, {len(out['cvae'])} cvae entries, top level {out['top_level_keys']}")


if __name__ == "__main__":
    torch.manual_seed(0)
    if len(sys.argv) > 1:                                 # e.g. `make_golden.py run_checkpoint_schema`: one fixture only
        for name in sys.argv[1:]:
            globals()[name]()
        sys.exit(0)
    run_graph_constants()
    run_variant("mocha24_g1", "mocha", seed=1777, gain=1.0, B=2)
    run_variant("mocha24_g2", "mocha", seed=4242, gain=2.0, B=1)
    run_variant("mixamo22_g1", "mixamo", seed=2222, gain=1.0, B=1)
    run_config_variants()
    run_match()
    run_cvae()
    run_featurize()
    run_featurize_mixamo()
    run_database()
    run_postprocess()
    run_postprocess_mixamo()
    run_bvh()
    run_checkpoint_schema()
