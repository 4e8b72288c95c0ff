#!/usr/bin/env python3
"""Prints the constant block of neuma_amd/csrc/nm_shrot.hip (between `// BEGIN generated tables` and `// END generated
tables`): the sample directions and A_l^{-1} of the SH rotation formula, from the torch function's own
`sh_rotation_tables` (neuma_amd/render/transform_utils.py).  tests/test_sh_rotation_cpu.py holds the two together.

    python tools/gen_shrot_tables.py          # paste the output over the block"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _rows(a):
    return ",\n".join("    " + ", ".join(f"{float(v)!r}" for v in row) for row in a)


def tables() -> str:
    from neuma_amd.render.transform_utils import sh_rotation_tables
    dirs, ainv = sh_rotation_tables()
    out = ["// unit sample directions s_k; band l uses the first 2l+1",
           "#define NM_SHROT_DIRS \\", _rows(dirs).replace("\n", " \\\n"),
           "// A_1^{-1} (3x3) | A_2^{-1} (5x5) | A_3^{-1} (7x7), each row-major [k][j], A_l[i][k] = Y_l,i(s_k)",
           "#define NM_SHROT_AINV \\", ", \\\n".join(_rows(a).replace("\n", " \\\n") for a in ainv)]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    sys.stdout.write(tables())
