"""CPU: the caller-QP layout of csrc/qsp_point.hpp, QpLaneData::has_structure and free_entries, compiled for the
host in a program of its own (tests/stubs/qp_layout_main.cpp) with the address and undefined-behaviour
sanitizers.  Nothing is loaded into Python.

The program forms a full 4 x 4 A with pack_lin (csrc/qsp_math.hpp: the library's own expansion of the six free
entries a = {a02, a03, a12, a13, a23, a33} of Lin, the order of the L_A fields) from a = 11 .. 16, and
perturbs it at each of the 16 positions in turn.  Exactly the six free positions may move without losing the
structure, by a finite amount or to NaN, and free_entries returns them in Lin's order."""
import subprocess

import host_program

FREE = {2: 0, 3: 1, 6: 2, 7: 3, 11: 4, 15: 5}      # row-major position of a02, a03, a12, a13, a23, a33 -> index in a
BASE = [11.0, 12.0, 13.0, 14.0, 15.0, 16.0]


def test_structure_and_free_entries(tmp_path):
    exe = host_program.build("qp_layout_main", tmp_path / "qp_layout_main")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[0] == "layout ok", r.stdout
    first = lines[1].split()
    assert first[0] == "1" and [float(v) for v in first[1:]] == BASE, lines[1]
    rows = [ln.split() for ln in lines[2:18]]
    assert [int(w[0]) for w in rows] == list(range(16))
    for p, w in enumerate(rows):
        finite_ok, nan_ok, a = int(w[1]), int(w[2]), [float(v) for v in w[3:]]
        want = list(BASE)
        if p in FREE:
            want[FREE[p]] += 0.5
        assert finite_ok == nan_ok == (1 if p in FREE else 0), (p, w)
        assert a == want, (p, a)
