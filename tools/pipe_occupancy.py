"""Diagnostics: the residency hipOccupancyMaxActiveBlocksPerMultiprocessor reports for the FFD kernels
of a load (stats build: fp_debug_pipe_occupancy), u32 kernel and packed twin, each with its own
dynamic LDS size.

    FLEETPLACE_LIB=$PWD/fleetflow_amd/libfleetplace_stats.so python tools/pipe_occupancy.py [S [C [N]]]
"""
import ctypes as ct
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("FLEETPLACE_LIB", os.path.join(ROOT, "fleetflow_amd", "libfleetplace_stats.so"))

from fleetflow_amd import Planner, _lib  # noqa: E402


def main():
    S, C, N = (int(a) for a in (sys.argv[1:4] + ["4096", "50000", "5000"][len(sys.argv) - 1:]))
    p = Planner(0)
    f = _lib.load().fp_debug_pipe_occupancy
    f.argtypes = [ct.c_void_p, ct.c_uint32, ct.c_uint32, ct.c_uint32, ct.POINTER(ct.c_int)]
    out = (ct.c_int * 5)()
    _lib.check(f(p._ctx, S, C, N, out), "fp_debug_pipe_occupancy")
    geo = p.geometry(S, C, N)
    print(f"S={S} C={C} N={N}: {geo['segments']} segments of {geo['stages']} stages x {geo['groups']} groups, "
          f"{S * geo['segments']} workgroups, {out[4]} compute units, FP_GEOM_RESIDENT {geo['resident']}")
    for name, occ, lds in (("u32", out[0], out[1]), ("packed", out[2], out[3])):
        if occ:
            waves = occ * geo["stages"]
            print(f"  {name:6s} kernel: {occ} workgroups per CU ({waves / 4:g} waves per SIMD) on {lds} B of dynamic LDS, "
                  f"{occ * out[4]} resident, {S * geo['segments'] / (occ * out[4]):.2f} rounds")


if __name__ == "__main__":
    main()
