"""A model file holds the output nonlinearity a fit trains with (1 sigmoid, 2 tanh); any other value is refused by the reader with a
message that names the file, before anything builds a network from it."""
import numpy as np
import pytest

import oracle


@pytest.mark.parametrize("out_act", [0, 3])
def test_model_file_refuses_an_output_nonlinearity_no_fit_has(tmp_path, out_act):
    from npp_amd import modelfile
    path = str(tmp_path / "model.npz")
    angles, periods, _ = oracle.synthetic_periodicity(64, 1)
    with pytest.raises(ValueError, match="out_act"):
        modelfile.write(path, oracle.init_params(1, W=256, seed=0), np.zeros(6, np.float32), angles, periods, oracle.SEED0_FREQS,
                        (64, 64), 256, out_act=out_act)
    modelfile.write(path, oracle.init_params(1, W=256, seed=0), np.zeros(6, np.float32), angles, periods, oracle.SEED0_FREQS,
                    (64, 64), 256, out_act=2)
    assert modelfile.read(path)["out_act"] == 2
    with np.load(path, allow_pickle=False) as f:
        arrays = {k: f[k] for k in f.files}
    arrays["npp/out_act"] = np.asarray(out_act, np.int64)
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, **arrays)
    with pytest.raises(ValueError, match=rf"bad\.npz: out_act = {out_act}"):
        modelfile.read(bad)
