"""GPU: bands/flow_gmflow.py with --corr_radius_list / --prop_radius_list (local matching, local-window propagation) on the clip of
tests/test_band_cli.py: the same outputs as the default run, another flow; radii outside the engine's are refused before the model loads."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bands"))

pytestmark = pytest.mark.gpu


def test_flow_gmflow_cli_local_radii(tmp_path):
    import flow_gmflow as band
    from prisma_amd import synth
    folder = tmp_path / "clip"
    folder.mkdir()
    frames = synth.frame_pair_sequence(4, 176, 256, seed=6)
    np.save(folder / "rgba.npy", frames)
    (folder / "metadata.json").write_text(json.dumps({"bands": {"rgba": {"url": "rgba.npy"}}}))
    os.environ["PRISMA_OVERWRITE"] = "1"
    band.model = None
    band.main(["-i", str(folder), "--scale", "1.0", "-b", "--mask"])
    default = np.load(folder / "flow_gmflow.npy")
    band.model.close()
    band.model = None
    # with a matching radius the reference raises on -b / --mask; the band computes the backward direction from the swapped pair
    band.main(["-i", str(folder), "--scale", "1.0", "--corr_radius_list", "4", "--prop_radius_list", "1", "-b", "--mask"])
    out = np.load(folder / "flow_gmflow.npy")
    assert out.shape == (4, 176, 256, 3) and out.dtype == np.uint8 and not out[-1].any() and out[0].any()
    assert not np.array_equal(out, default)
    for other in ("flow_gmflow_bwd.npy", "flow_gmflow_mask.npy", "flow_gmflow_mask_bwd.npy"):
        assert np.load(folder / other).shape == out.shape, other
    assert np.load(folder / "flow_gmflow_bwd.npy")[0].any()
    dist = [float(x) for x in open(folder / "flow_gmflow.csv")]
    assert len(dist) == 4 and dist[-1] == 0.0 and all(d > 0 for d in dist[:-1])
    md = json.load(open(folder / "metadata.json"))
    assert md["bands"]["flow_gmflow"]["values"]["dist"] == {"type": "float", "url": "flow_gmflow.csv"}
    band.model.close()
    band.model = None
    for flags in (["--corr_radius_list", "5"], ["--corr_radius_list", "0"], ["--prop_radius_list", "3"], ["--corr_radius_list", "-1", "4"],
                  ["--prop_radius_list", "-1", "1"]):
        with pytest.raises(SystemExit, match="takes one radius"):
            band.main(["-i", str(folder)] + flags)
        assert band.model is None                       # refused before the model loads
    with pytest.raises(SystemExit, match="only the band's default GMFlow"):
        band.main(["-i", str(folder), "--corr_radius_list", "4", "--attn_splits_list", "1"])
