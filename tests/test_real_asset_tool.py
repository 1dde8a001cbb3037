"""tools/real_asset_parity.py: real-asset parity in one command, validated today on a checkpoint FILE in the
reference Trainer's schema with synthetic weights.

* GPU (-m gpu): the `replay` half loads a checkpoint file through the C ABI host and replays the committed reference
  fixture generator_mocha24_g2.npz (gain 2: outputs of a trained model's size) stage by stage against 1e-4.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


def _write_trainer_schema_file(path, sd, prefix=""):
    t = {prefix + k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    p = [torch.nn.Parameter(torch.zeros(3))]
    torch.save({"gen": t, "gen_ema": t, "gen_opt": torch.optim.AdamW(p, lr=1e-4).state_dict()}, path)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_replay_half_on_a_trainer_schema_file_against_the_reference_fixture(tmp_path, golden_dir, capsys):
    import real_asset_parity as R
    from mocha_sigasia2023_amd import weights
    ckpt = str(tmp_path / "gen_125.pt")
    _write_trainer_schema_file(ckpt, weights.synthetic_state_dict(4242, 2.0, "mocha"), prefix="module.")
    rc = R.main(["replay", "--ckpt", ckpt, "--fixture", os.path.join(golden_dir, "generator_mocha24_g2.npz")])
    text = capsys.readouterr().out
    assert rc == 0, text
    assert "RESULT:" in text and "PASS" in text and "ABOVE" not in text
    for stage in ("src.mot_embedding", "cha.encoder", "decoder", "to_mot", "end to end (own encoder outputs) Y"):
        assert stage in text
    # a checkpoint that is not the fixture's: refused by hash when the fixture records one
    fx = dict(np.load(os.path.join(golden_dir, "generator_mocha24_g2.npz")))
    fx["meta"] = np.array(json.dumps({"layout": "mocha", "ckpt_sha256": "0" * 64}))
    other = str(tmp_path / "other.npz")
    np.savez(other, **fx)
    assert R.main(["replay", "--ckpt", ckpt, "--fixture", other]) == 2
