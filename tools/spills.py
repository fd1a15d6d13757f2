"""List register spills / scratch of every kernel in the built library's gfx950 code objects.

    python tools/spills.py [--all]      (reads picotron_amd/lib/obj/*.o; exit 1 if any kernel spills)

Each object's gfx950 code object is unbundled and its AMDGPU metadata notes are read
(tools/codeobj.py): .vgpr_spill_count, .sgpr_spill_count and .private_segment_fixed_size (scratch
bytes per lane) per kernel."""
import glob
import os
import sys

from codeobj import ROOT, kernels


def main():
    show_all = "--all" in sys.argv
    bad = 0
    for obj in sorted(glob.glob(os.path.join(ROOT, "picotron_amd", "lib", "obj", "*.o"))):
        for k in kernels(obj):
            spill = k["vspill"] or k["scratch"]   # SGPR spills go to VGPR lanes (v_writelane), not memory
            bad += bool(spill)
            if spill or show_all or k["sspill"]:
                print(f"{os.path.basename(obj):18s} vgpr={k['vgpr']:3d} agpr={k['agpr']:3d} vspill={k['vspill']:3d} "
                      f"sspill={k['sspill']:3d} scratch={k['scratch']:4d} lds={k['lds']:6d} {k['name'][:120]}")
    print(f"{bad} kernel(s) with VGPR spills or scratch memory")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
