"""How often a wave-step of the trace kernel is not the calm step: run the trace with a -DCBET_DIAG_FACES build of the
library (scripts/variants/diag_faces.flags; CBET_LIB_PATH must point at it).  That build counts, per wave-step, whether the
step starts near a face (some axis of the per-axis mask set: the general relocation and the exit planes run), how many axes
are near, and whether the step enters the window arm, and reports the sums through four of the counter slots.
usage: CBET_LIB_PATH=build_alt/libcbet_diag_faces.so python scripts/face_share.py [n=256] [out.json]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cbet_raytracing_3d_amd import api                      # noqa: E402
from cbet_raytracing_3d_amd.tracer import RayTracer         # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
if "diag_faces" not in os.environ.get("CBET_LIB_PATH", ""):
    raise SystemExit("set CBET_LIB_PATH to the -DCBET_DIAG_FACES build")
r, ne, te = api.load_s83177()
tr = RayTracer(api.default_params(n), r, ne, te)
e = tr.new_grid(zpitch=True)
tr.counters(reset=True)
tr.launch(e)
torch.cuda.synchronize()
c = tr.counters(reset=True)
ws = float(c.wave_steps)
out = dict(n=n, ray_steps=int(c.ray_steps), wave_steps=int(c.wave_steps), near_steps=int(c.wave_steps_wide),
           near_axes=int(c.wave_steps_miss), window_arm_steps=int(c.slabs_retired),
           near_share=c.wave_steps_wide / ws, window_arm_share=c.slabs_retired / ws,
           axes_per_near_step=c.wave_steps_miss / max(1.0, float(c.wave_steps_wide)))
print("%d^3: %.4g wave-steps; near a face %.2f %% (%.2f axes each where the build counts them); window arm %.2f %%"
      % (n, ws, 100 * out["near_share"], out["axes_per_near_step"], 100 * out["window_arm_share"]))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
