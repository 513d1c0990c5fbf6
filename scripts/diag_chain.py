"""The length of the trace kernel's dependent chain, measured with the shader clock inside the kernel: run the 256^3 trace
with a -DCBET_DIAG_CHAIN build of the library (scripts/variants/diag_chain.flags; CBET_LIB_PATH must point at it).  That
build stamps s_memtime right behind the record wait and right behind the issue of the next step's gather and sums the
difference per wave: record arrives -> kick -> move -> relocate -> gather.  Each stamp is a scalar-memory read and an
lgkmcnt(0) wait, the first of them ON the chain, so the figure is not the shipped kernel's: compare builds that carry the
same stamps with each other only (scripts/variants/chain_diag_parent.* is the parent commit with them).
usage: CBET_LIB_PATH=build_alt/libcbet_diag_chain.so python scripts/diag_chain.py [n=256]      (prints one JSON line last)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cbet_raytracing_3d_amd import api                      # noqa: E402
from cbet_raytracing_3d_amd.tracer import RayTracer         # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
if "diag" not in os.environ.get("CBET_LIB_PATH", ""):
    raise SystemExit("set CBET_LIB_PATH to a -DCBET_DIAG_CHAIN build")
r, ne, te = api.load_s83177()
tr = RayTracer(api.default_params(n), r, ne, te)
e = tr.new_grid(zpitch=True)
for k in range(3):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e.zero_()
    tr.counters(reset=True)
    a.record()
    tr.launch(e)
    b.record()
    torch.cuda.synchronize()
c = tr.counters(reset=True)
ws, cycles = float(c.wave_steps), float(c.global_atomics)
print("diag build: launch %.2f ms, %d ray-steps, %.4g wave-steps" % (a.elapsed_time(b), c.ray_steps, ws))
print("record wait -> next gather issued: %.1f shader clocks per wave-step" % (cycles / ws))
print(json.dumps({"library": os.path.basename(os.environ["CBET_LIB_PATH"]), "n": n, "launch_ms": a.elapsed_time(b),
                  "ray_steps": int(c.ray_steps), "wave_steps": int(c.wave_steps), "chain_clocks": int(c.global_atomics),
                  "chain_clocks_per_wave_step": cycles / ws}))
