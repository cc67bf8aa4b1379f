"""The F(4,3) operand writer (modulate_wino4_kernel, csrc/i2v_dec_writers.hip) stores whole 16-byte pieces after a DPP exchange between the two
lanes of a pair (form 1); the measurement build also holds the form that requests the next input frame ahead of the current frame's
stores (3) and the earlier 8-byte stores (0), selected by I2V_MOD4_FORM.  No form changes a byte of V: tests/writer_forms_worker.py
-- in a process of its own, on that build -- compares the tapped operands (into NaN-filled buffers) and the frames of every form
against those of form 0, byte for byte, and checks that the switch reached the launch.

Configs: B = 2, nf = 32; up-sampling plans ([2, 1], [2, 1]) and ([2, 2], [2, 1]).  Together: W = 16 (J = 4: a wave's 16-tile segment
spans four (h, chunk) rows), W = 32 / 64 / 128 (two and more segments per row: left_own and right_own), C = 32 / 64 / 128 ..., ut and us
1 and 2, the SPADE form (conv_0), the ADAIN form (conv_1), the shared-map form (realizations = 3) and the one-term form ("fp16")."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ups,upt,img,widths", [([2, 1], [2, 1], 64, {16, 32, 64}), ([2, 2], [2, 1], 128, {16, 32, 64, 128})])
def test_writer_forms_write_the_same_bytes(ups, upt, img, widths):
    import i2v_native
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    if not os.path.exists(i2v_native.MEASURE_LIB_PATH):
        i2v_native.build_measure()
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, I2V_LIB_PATH=os.path.join("image2video-synthesis-using-cinns_amd", "lib", "libi2v_hip_measure.so"))   # relative to the repo root
    env.pop("I2V_MOD4_FORM", None)
    r = subprocess.run([sys.executable, os.path.join(repo, "tests", "writer_forms_worker.py"),
                        json.dumps({"upsample_s": ups, "upsample_t": upt, "img": img})], env=env, cwd=repo, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["bad"] == [], res
    assert res["checked"] >= 4 * 3 * 3, res                      # four modes x three forms x (frames + at least two taps)
    shapes = [tuple(s) for s in res["shapes"]]
    assert {w for w, _, _ in shapes} >= widths, shapes
    assert {c for _, c, _ in shapes} >= {32, 64, 128}, shapes
    assert {which for _, _, which in shapes} == {1, 3}, shapes
