"""The global-tour solver without a GPU: the restatement (tests/tsp_ref.py) against brute force and the reference's
file route, the ILS's rules, the C-ABI (header, exports, struct layout, ENODEV), the Python conversion, and the
drop-in libfuelmi_lkh.so (its export, what the reference's exploration manager imports, its refusals)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tsp_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fuelmi.h")
LKH_LIB = os.path.join(ROOT, "fuel_amd", "libfuelmi_lkh.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dropin_lkh_imports.txt")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import fuel_amd
    return fuel_amd


# ---- the exact method -----------------------------------------------------------------------------------------------------
def _matrices(rng, d):
    big = (2 ** 31 - 1) // d
    return [rng.integers(0, 100, (d, d)), np.full((d, d), 5), np.zeros((d, d), np.int64),
            rng.integers(-100, 100, (d, d)), rng.integers(big - 10, big, (d, d)), rng.integers(0, 2, (d, d))]


@pytest.mark.parametrize("d", range(2, 9))
def test_held_karp_is_the_smallest_optimal_order(d):
    rng = np.random.default_rng(d)
    for c in _matrices(rng, d):
        o, v = tr.held_karp(c)
        bo, bv = tr.brute_force(c)
        assert (o, v) == (bo, bv), (c, o, v, bo, bv)
        if (c == c.flat[0]).all():
            assert o == list(range(d))


def test_overflow_needs_int64():
    d = 8
    big = (2 ** 31 - 1) // d
    c = np.full((d, d), big - 1)
    o, v = tr.held_karp(c)
    assert v == d * (big - 1) and v > 2 ** 31 - 1 - d * 2 and o == list(range(d))
    assert tr.held_karp(np.full((d, d), 2 ** 31 - 1))[1] == d * (2 ** 31 - 1)  # beyond int32 in every sum


def test_special_dimensions():
    assert tr.held_karp(np.array([[42]])) == ([0], 0)
    assert tr.held_karp(np.array([[9, 3], [4, 9]])) == ([0, 1], 7)


# ---- the heuristic --------------------------------------------------------------------------------------------------------
def test_move_deltas_are_cost_differences():
    rng = np.random.default_rng(4)
    for d in (5, 6, 11, 18):
        c = rng.integers(-100, 1000, (d, d))
        o = [0] + rng.permutation(np.arange(1, d)).tolist()
        base = tr.tour_cost(c, o)
        delta, key = tr.move_deltas(c, o)
        assert len(set(key.tolist())) == len(key)
        n2 = (d - 1) * (d - 2) // 2
        assert (key[:n2] < 6 * d * d).all() and (key[n2:] >= 6 * d * d).all()
        for dv, kv in zip(delta, key):
            n = tr.apply_move(o, int(kv))
            assert n[0] == 0 and sorted(n) == list(range(d))
            assert tr.tour_cost(c, n) - base == dv


def test_kick_points_and_double_bridge():
    for d in (5, 6, 40, 1024):
        for r in range(4):
            for k in range(6):
                p = tr.kick_points(7, r, k, d)
                assert 1 <= p[0] < p[1] < p[2] <= d - 1
    assert tr.kick_points(7, 1, 2, 100) == tr.kick_points(7, 1, 2, 100)
    assert tr.kick_points(7, 1, 2, 100) != tr.kick_points(8, 1, 2, 100)
    assert tr.double_bridge(list(range(8)), 2, 4, 7) == [0, 1, 4, 5, 6, 2, 3, 7]
    assert tr.mix(0) == 0xE220A8397B1DCDAF  # splitmix64's first output from state 0


def test_ils_is_deterministic_and_locally_optimal():
    rng = np.random.default_rng(3)
    for d in (14, 30, 50):
        c = rng.integers(0, 1000, (d, d))
        a = tr.ils(c, 3, 4, 11)
        b = tr.ils(c, 3, 4, 11)
        assert a == b
        o, v = a
        assert o[0] == 0 and sorted(o) == list(range(d)) and tr.tour_cost(c, o) == v
        assert tr.local_optimum_violations(c, o) == []
        assert v <= tr.local_search(c, tr.nearest_neighbour(c))[1]
    # on small instances it reaches the optimum often; never below it
    for d in (6, 7, 8):
        c = rng.integers(0, 50, (d, d))
        assert tr.ils(c, 2, 3, 0)[1] >= tr.held_karp(c)[1]


def test_nearest_neighbour_ties_to_smallest_index():
    c = np.array([[0, 5, 1, 1], [1, 0, 1, 1], [3, 3, 0, 3], [1, 1, 1, 0]])
    assert tr.nearest_neighbour(c) == [0, 2, 1, 3]


# ---- the reference's file route ---------------------------------------------------------------------------------------------
def test_reference_writer_and_reader():
    m = np.array([[0.0, 1.239, -2.5], [0.0, 0.0, 3.999], [0.0, 7.0, 0.0]])
    assert tr.ref_int_matrix(m) == [[0, 123, -250], [0, 0, 399], [0, 700, 0]]
    text = tr.write_tsp(m)
    assert text.startswith("NAME : single\nTYPE : ATSP\nDIMENSION : 3\nEDGE_WEIGHT_TYPE : EXPLICIT\n"
                           "EDGE_WEIGHT_FORMAT : FULL_MATRIX\nEDGE_WEIGHT_SECTION\n0 123 -250 \n")
    assert text.endswith("0 700 0 \nEOF")
    tour = "NAME : single.5.tour\nCOMMENT : Length = 5\nTYPE : TOUR\nDIMENSION : 3\nTOUR_SECTION\n1\n3\n2\n-1\nEOF\n"
    assert tr.read_tour(tour) == [1, 0]


def test_tour_matrix_truncates_and_refuses():
    import fuel_amd
    m = np.array([[0.0, 1.239, -2.5], [0.0, 0.0, 3.999], [0.0, 21474836.47, 0.0]])
    assert np.array_equal(fuel_amd.tour_matrix(m), np.array(tr.ref_int_matrix(m)))
    assert fuel_amd.tour_matrix(m).dtype == np.int32
    for bad in (np.nan, np.inf, 21474836.48, -21474836.48):
        mm = m.copy()
        mm[1, 2] = bad
        with pytest.raises(ValueError):
            fuel_amd.tour_matrix(mm)
    with pytest.raises(ValueError):
        fuel_amd.tour_matrix(np.zeros((2, 3)))


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def test_header_declares_tsp_and_library_exports_it(built):
    src = open(HEADER).read()
    assert re.search(r"typedef struct \{\s*int restarts, kicks, exact_max;\s*uint64_t seed;\s*\} fuelmi_tsp_cfg;", src)
    assert "int fuelmi_tsp_create(int device, const fuelmi_tsp_cfg* cfg, fuelmi_tsp** out);" in src
    assert "void fuelmi_tsp_destroy(fuelmi_tsp* t);" in src
    assert re.search(r"int fuelmi_tsp_solve\(fuelmi_tsp\* t, int n_prob, const int\* dim_ptr, const int32_t\* costs, "
                     r"int\* order,\s*int64_t\* tour_cost, int\* method\);", src)
    assert "#define FUELMI_TSP_MAX_DIM 1024" in src
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH]).decode()
    for name in ("fuelmi_tsp_create", "fuelmi_tsp_destroy", "fuelmi_tsp_solve"):
        assert re.search(r" T %s$" % name, out, flags=re.M), name


def test_tsp_cfg_layout_matches_c(built, tmp_path):
    from fuel_amd import _lib
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fuelmi.h"\n'
                    'int main(){printf("%zu %zu %d %d %d %d %d\\n", sizeof(fuelmi_tsp_cfg), offsetof(fuelmi_tsp_cfg, seed), '
                    'FUELMI_TSP_MAX_DIM, FUELMI_TSP_EXACT_CAP, FUELMI_TSP_DEFAULT_RESTARTS, FUELMI_TSP_DEFAULT_KICKS, '
                    'FUELMI_TSP_DEFAULT_EXACT_MAX);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T = _lib.TspCfg
    assert got == [C.sizeof(T), T.seed.offset, _lib.TSP_MAX_DIM, _lib.TSP_EXACT_CAP, _lib.TSP_DEFAULT_RESTARTS,
                   _lib.TSP_DEFAULT_KICKS, _lib.TSP_DEFAULT_EXACT_MAX]


def test_create_refuses_config_and_needs_a_gfx950_device(built):
    from fuel_amd import _lib
    L = built.lib()
    for cfg in ((0, 5, 12), (4, -1, 12), (4, 5, 2), (4, 5, 17)):
        h = C.c_void_p(99)
        assert L.fuelmi_tsp_create(0, C.byref(_lib.TspCfg(*cfg, 0)), C.byref(h)) == -1, cfg
        assert h.value == 99
    h = C.c_void_p(99)
    rc = L.fuelmi_tsp_create(0, C.byref(_lib.TspCfg(4, 5, 12, 0)), C.byref(h))
    if L.fuelmi_device_count() == 0:
        assert rc == -2 and h.value == 99  # FUELMI_ENODEV, nothing created
    else:  # (the same suite on a GPU box)
        assert rc in (0, -2)
        if rc == 0:
            L.fuelmi_tsp_destroy(h)
    assert L.fuelmi_tsp_solve(None, 1, None, None, None, None, None) == -1


# ---- the drop-in libfuelmi_lkh.so ---------------------------------------------------------------------------------------
def test_lkh_library_exports_what_the_exploration_manager_imports(built):
    need = [tuple(l.rstrip("\n").split("\t", 1)) for l in open(GOLDEN) if l.strip()]
    assert need == [("_Z11solveTSPLKHPKc", "solveTSPLKH(char const*)")]
    have = {l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", LKH_LIB]).decode().splitlines()}
    assert "_Z11solveTSPLKHPKc" in have
    # it stays out of the facade library, whose links are unchanged
    fac = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "fuel_amd", "libfuelmi_facade.so")])
    assert b"solveTSPLKH" not in fac
    # where the reference checkout is present, the live drop-in object imports exactly that
    obj = os.path.join(ROOT, "build", "dropin", "fast_exploration_manager.o")
    if os.path.exists(obj):
        import importlib.util
        spec = importlib.util.spec_from_file_location("mk", os.path.join(ROOT, "tests", "golden", "make_dropin_lkh_golden.py"))
        mk = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mk)
        assert mk.lkh_imports(obj) == need


def _lkh(par):
    L = C.CDLL(LKH_LIB)
    fn = getattr(L, "_Z11solveTSPLKHPKc")
    fn.restype, fn.argtypes = C.c_int, [C.c_char_p]
    return fn(str(par).encode())


def _problem(d=3, **over):
    hdr = dict(NAME="single", TYPE="ATSP", DIMENSION=str(d), EDGE_WEIGHT_TYPE="EXPLICIT",
               EDGE_WEIGHT_FORMAT="FULL_MATRIX")
    hdr.update(over)
    s = "".join("%s : %s\n" % (k, v) for k, v in hdr.items() if v is not None) + "EDGE_WEIGHT_SECTION\n"
    return s + "".join("".join("%d " % ((i * 7 + j) % 5) for j in range(d)) + "\n" for i in range(d)) + "EOF"


@pytest.mark.parametrize("case", ["type", "format", "weight_type", "dimension", "short", "long", "no_eof", "key",
                                  "no_problem", "missing_file"])
def test_lkh_refusals_remove_the_tour_files(built, tmp_path, case):
    par, tsp, out, tour = tmp_path / "single.par", tmp_path / "single.tsp", tmp_path / "single.txt", tmp_path / "t2.txt"
    text = {"type": _problem(TYPE="TSP"), "format": _problem(EDGE_WEIGHT_FORMAT="LOWER_ROW"),
            "weight_type": _problem(EDGE_WEIGHT_TYPE="EUC_2D"), "dimension": _problem(DIMENSION="1025"),
            "short": _problem().replace("EOF", "").rsplit(" ", 2)[0] + "\nEOF",
            "long": _problem().replace("EOF", "4 EOF"), "no_eof": _problem().replace("EOF", ""),
            "key": _problem(CAPACITY="3")}.get(case, _problem())
    tsp.write_text(text)
    lines = ["output_tour_file = %s" % out, "TOUR_FILE=%s" % tour, "RUNS = 1", "# a comment"]
    if case != "no_problem":
        lines.insert(0, "Problem_File = %s" % (tsp if case != "missing_file" else tmp_path / "nothing.tsp"))
    par.write_text("\n".join(lines) + "\n")
    out.write_text("TOUR_SECTION\n1\n2\n3\n-1\nEOF\n")  # last cycle's tour
    tour.write_text("stale")
    assert _lkh(par) != 0
    assert not out.exists() and not tour.exists()
