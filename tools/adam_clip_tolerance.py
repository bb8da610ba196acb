"""The accuracy of the clip-and-Adam contract (mhppo.adam.adam_clip_torch = mhppo_adam_clip) and of
today's float32 path, both against float64: clip_grad_norm_ + torch.optim.Adam on float64 CPU copies,
three steps, six nets of the product's sizes, max_norm between the nets' norms
(tests/adam_clip_common.py accuracy_case).  error = |d| / max(1, |ref|) over all parameters.
tests/adam_clip_common.py YARDSTICK_WORST is the float32 path's figure; the contract may be 4x it.

usage: python tools/adam_clip_tolerance.py > profiles/adam_clip/tolerance.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mh-ppo_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import adam_clip_common as C  # noqa: E402

params, grads = C.accuracy_case()
ref, ref_norms = C.torch_path(params, grads, torch.float64)
f32, _ = C.torch_path(params, grads, torch.float32)
spec, spec_norms = C.spec_path(params, grads)
print(f"torch {torch.__version__}, {C.ACC_STEPS} steps, nets {C.PRODUCT_NETS}, max_norm {C.ACC_MAX_NORM}")
for t, row in enumerate(ref_norms, 1):
    print(f"step {t}: float64 norms " + " ".join(f"{x:.4f}" for x in row)
          + f"   clipped {sum(x > C.ACC_MAX_NORM for x in row)} of {len(row)}")
rel = max(abs(a - b) / b for ra, rb in zip(spec_norms, ref_norms) for a, b in zip(ra, rb))
print(f"contract's norms against the float64 reference's: worst relative gap {rel:.3e}")
for name, got in (("float32 torch path (yardstick)", f32), ("contract (adam_clip_torch)", spec)):
    per = " ".join(f"{C.worst_error([g], [r]):.3e}" for g, r in zip(got, ref))
    print(f"{name:32s} worst {C.worst_error(got, ref):.3e}   per net {per}")
print(f"bound of tests/test_adam_clip_host.py: 4 x {C.YARDSTICK_WORST:.3e} = {4 * C.YARDSTICK_WORST:.3e}")
