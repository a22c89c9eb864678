#!/usr/bin/env python3
"""Generate tests/golden/manifest_wire_isa.json: the SHA-256 of every input
table of tests/wire_tables.py and of what the x86 instructions of the wire
casts (oracle/isa_wire.cpp through oracle.IsaWire) give on them.

Producer: the CPU itself -- vcvtps2ph (imm8 = 0), vcvtph2ps, packssdw,
vpmovsxwd, vcvttss2si and the uint16 -> float conversion, one function each,
compiled with the oracle's flags.  tests/test_wire_isa_host.py recomputes both
sets of digests, so a change of the tables, or a CPU / compiler on which the
yardstick itself computes something else, is noticed before any comparison
against it is believed.

    python tests/golden/make_golden_wire_isa.py
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import wire_tables as T  # noqa: E402
from oracle.oracle import IsaWire  # noqa: E402


def main():
    isa = IsaWire()
    out = {"producer": "x86 instructions of the wire casts executed on the CPU (oracle/isa_wire.cpp, "
                       "-O3 -march=broadwell): _mm256_cvtps_ph(v, 0), _mm256_cvtph_ps, _mm_packs_epi32, "
                       "_mm256_cvtepi16_epi32, (uint16_t)_mm_cvttss_si32, (float)uint16_t",
           "sizes": {"F32_BOUNDARY": int(T.f32_boundary().size), "F16_ALL": int(T.F16_ALL.size),
                     "TAIL_F32": int(T.TAIL_F32.size), "IDX_U32": int(T.IDX_U32.size),
                     "TAIL_U16": int(T.TAIL_U16.size)},
           "tables": T.table_digests(), "instructions": T.isa_digests(isa)}
    with open(os.path.join(HERE, "manifest_wire_isa.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for k, v in out["sizes"].items():
        print(k, v)


if __name__ == "__main__":
    main()
