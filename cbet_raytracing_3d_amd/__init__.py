"""cbet_raytracing_3d_amd -- MI355X-native ray integrator behind the C ABI of include/cbet_mi355x.h.

api     ctypes binding of libcbet_mi355x.so (no CPU fallback; raises if the library is missing)
tracer  RayTracer: torch-held device buffers around the launches; re-exports the three modules below
pipeline   the plain path's grid combine and SweepPipeline (torch.distributed / RCCL)
cbet_loop  the CBET fixed-point loops and their device engine
exchange   the slab-owned loop's exchange over point-to-point links
modes, lpi what is derived from mode spectra and from the quarter-critical LPI maps
build   hipcc build of the library for gfx950
"""
__all__ = ["api", "tracer", "build"]
