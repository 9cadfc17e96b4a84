"""bands/flow_gmflow.py and the refinement model's flag set (--num_scales 2 --upsample_factor 4 --padding_factor 32 --attn_splits_list 2 8
--corr_radius_list -1 R --prop_radius_list -1 r): what is refused is refused before the model loads (CPU), a flags / checkpoint mismatch
before anything runs, and (GPU) the full flag set with --synthetic weights writes the band's usual outputs."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bands"))

REFINE = ["--num_scales", "2", "--upsample_factor", "4", "--padding_factor", "32", "--attn_splits_list", "2", "8", "--corr_radius_list", "-1", "4",
          "--prop_radius_list", "-1", "1"]


def clip(tmp_path, n=3, h=72, w=104):
    from prisma_amd import synth
    folder = tmp_path / "clip"
    folder.mkdir()
    np.save(folder / "rgba.npy", synth.frame_pair_sequence(n, h, w, seed=6))
    (folder / "metadata.json").write_text(json.dumps({"bands": {"rgba": {"url": "rgba.npy"}}}))
    os.environ["PRISMA_OVERWRITE"] = "1"
    return folder


def drop(flags, name, n):
    i = flags.index(name)
    return flags[:i] + flags[i + 1 + n:]


def test_refusals_before_the_model_loads(tmp_path):
    import flow_gmflow as band
    folder = clip(tmp_path)
    band.model = None
    default = "only the band's default GMFlow"
    cases = [(["--num_scales", "2"], default),                                                 # on its own: its lists have one entry
             (drop(REFINE, "--upsample_factor", 1), default), (drop(REFINE, "--padding_factor", 1), default),
             (drop(REFINE, "--attn_splits_list", 2), default), (drop(REFINE, "--corr_radius_list", 2), default),
             (REFINE[:-1] + ["3"], default), (REFINE[:-1] + ["-1"], default),                  # r = 3, r = -1
             (REFINE + ["--inference_size", "80", "96"], "multiples of 32"),
             (REFINE + ["--num_head", "2"], default), (REFINE + ["--feature_channels", "64"], default),   # the other architecture flags stay checked
             (REFINE + ["--attention_type", "full"], default), (REFINE + ["--ffn_dim_expansion", "2"], default),
             (REFINE + ["--num_transformer_layers", "12"], default),
             (["--corr_radius_list", "-1", "4"], "takes one radius"), (["--prop_radius_list", "-1", "1"], "takes one radius"),
             (["--attn_splits_list", "1"], default), (["--attn_splits_list", "2", "8"], default), (["--upsample_factor", "4"], default)]
    for flags, text in cases:
        with pytest.raises(SystemExit, match=text):
            band.main(["-i", str(folder)] + flags)
        assert band.model is None, flags
    assert band.two_scale(band.argparse.Namespace(num_scales=2, upsample_factor=4, padding_factor=32, attn_splits_list=[2, 8],
                                                  corr_radius_list=[-1, 2], prop_radius_list=[-1, 2]))


def test_flags_and_checkpoint_must_agree(tmp_path, monkeypatch):
    """a one-scale checkpoint under the refinement flags and a two-scale one under the default flags are refused before an engine exists"""
    import flow_gmflow as band
    from prisma_amd import synth
    folder = clip(tmp_path)
    band.model = None
    made = []
    monkeypatch.setattr(band.engine, "FlowGMFlow", lambda *a, **k: made.append(1))
    for scales, flags in ((1, REFINE), (2, [])):
        monkeypatch.setattr(band, "load_weights", lambda path, s=scales: synth.gmflow_weights(seed=2468, num_scales=s))
        with pytest.raises(SystemExit, match="-scale model but the checkpoint is a"):
            band.main(["-i", str(folder)] + flags)
        assert band.model is None and not made


@pytest.mark.gpu
def test_flow_gmflow_cli_refinement_flags(tmp_path):
    import flow_gmflow as band
    folder = clip(tmp_path, 3, 100, 150)
    band.model = None
    band.main(["-i", str(folder), "--scale", "1.0", "--synthetic", "-b", "--mask"] + REFINE)
    assert band.model.num_scales == 2
    out = np.load(folder / "flow_gmflow.npy")
    assert out.shape == (3, 100, 150, 3) and out.dtype == np.uint8 and not out[-1].any() and out[0].any()
    for other in ("flow_gmflow_bwd.npy", "flow_gmflow_mask.npy", "flow_gmflow_mask_bwd.npy"):
        assert np.load(folder / other).shape == out.shape, other
    assert np.load(folder / "flow_gmflow_bwd.npy")[0].any()
    dist = [float(x) for x in open(folder / "flow_gmflow.csv")]
    assert len(dist) == 3 and dist[-1] == 0.0 and all(d > 0 for d in dist[:-1])
    md = json.load(open(folder / "metadata.json"))
    assert md["bands"]["flow_gmflow"]["values"]["dist"] == {"type": "float", "url": "flow_gmflow.csv"}
    band.model.close()
    band.model = None
    band.main(["-i", str(folder), "--scale", "1.0", "--synthetic"])                      # the default model afterwards, in the same process
    assert band.model.num_scales == 1 and not np.array_equal(np.load(folder / "flow_gmflow.npy"), out)
    band.model.close()
    band.model = None
