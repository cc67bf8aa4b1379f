"""Worker of tests/test_gpu_dec_rest.py::test_conv_img_forced_frames_per_workgroup_keep_the_bits: runs in a process of its own with
I2V_LIB_PATH on the MEASUREMENT build of the library, the only build that reads I2V_CONVIMG_TCH (output frames one workgroup of the fused
conv_img kernel keeps its brick for).  C = 32, (1, 16, 8, 32): 1, 2, 4, 8 and 16 frames per workgroup; JSON on the last stdout line."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "image2video-synthesis-using-cinns_amd")):
    sys.path.insert(0, p)
import dec_rest_common as dr  # noqa: E402
import i2v_native  # noqa: E402

assert os.path.basename(i2v_native.LIB_PATH) == "libi2v_hip_measure.so", i2v_native.LIB_PATH
torch.set_grad_enabled(False)
C, shape = 32, (1, 16, 8, 32)
x, w, bias = dr.conv_img_inputs(*shape, C, 1616)
xg = x.cuda()
outs, tchs, flags = [], [], 0
for t in (1, 2, 4, 8, 16):
    os.environ["I2V_CONVIMG_TCH"] = str(t)
    info = {}
    outs.append(i2v_native.conv_img_unit(xg, w, bias, form="mfma", info=info))
    tchs.append(info["tch"])
    flags |= info["range_flag"]
os.environ.pop("I2V_CONVIMG_TCH")
ref, S, S1, SW = dr.conv_img_ref(xg, w, bias)
fraction = dr.within(outs[0], ref, dr.conv_img_bound("mfma", C, w, ref, S, S1, SW), rel=0.0)
print(json.dumps({"tch": tchs, "equal": [bool(torch.equal(o, outs[0])) for o in outs[1:]], "range_flag": flags, "fraction": fraction,
                  "saturated": dr.saturated_share(ref)}))
