"""The sextet op table (csrc/dev/devcheck_sx.h) on the six-thread host
emulation against the Fp12 references of tests/sx_ref.py (CPU tier).

The emulation runs the sq_* routines of dev/sx29.h themselves, one job per six
threads with a real barrier, on the words the device tool reads
(tests/test_gpu_sx_ops.py).  Passing here validates the vectors, the packing,
the references and the bounds taken from the header, so that a failure of the
device test can only be the device's: its LDS exchange, barriers, ghost lanes
or compiled lane-role selects.  Every comparison is exact (value mod p); every
result's limbs 0..7 are balanced and its value within the bound its routine
states (sx_ref.OUT_BOUND cites each).
"""
import ctypes
import struct

import pytest
from conftest import build_emu

import sx_ref as R


@pytest.fixture(scope="module")
def emu_sx():
    lib = ctypes.CDLL(build_emu())
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.sxe_sx_info.argtypes = [ctypes.c_int, ctypes.c_char_p, u32p, u32p, u32p, u32p]
    lib.sxe_sx_ops.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p]
    return lib


def read_table(info):
    """an info entry point's table: name -> (index, nin, nout, slots, bofs)"""
    name = ctypes.create_string_buffer(32)
    v = [ctypes.c_uint32() for _ in range(4)]
    out = {}
    for i in range(info(-1, name, *v)):
        info(i, name, *v)
        out[name.value.decode()] = (i,) + tuple(x.value for x in v)
    return out


@pytest.fixture(scope="module")
def table(emu_sx):
    return read_table(emu_sx.sxe_sx_info)


def test_every_sx_op_has_vectors(table):
    """an op added to the header's table without vectors, a reference and mutants fails here"""
    assert set(table) == set(R.OPS), set(table) ^ set(R.OPS)
    assert sorted(t[0] for t in table.values()) == list(range(len(table)))
    with_mutants = {m[0] for m in R.MUTANTS}
    for name, (_, nin, nout, slots, bofs) in table.items():
        o = R.OPS[name]
        assert (o.nin, o.nout) == (nin, nout) and R.LAYOUT[name] == (slots, bofs), name
        assert name in R.OUT_BOUND and name in R.IN_BOUND and name in with_mutants, name
        vs = o.vectors()
        assert len(vs) == R.N_JOBS and R.N_JOBS % 10 and max(R.JOB_COUNTS) < R.N_JOBS, name
        assert all(R.operand_in_contract(name, v) for v in vs), name
        for w in range(0, R.N_JOBS, 10):  # the ten sextets of a wave hold different operands
            assert len(set(vs[w:w + 10])) == len(vs[w:w + 10]), name
    assert table["sx_mulv24"][3:] == (24, 12) and table["sx_expt"][3:] == (24, 12)  # k_fexp_expt's layout


def test_vectors_reach_the_contract():
    """the representatives the header allows are present: limbs at +2^28 and -2^28, values shifted by p up to the
    routine's bound, units, and both values of every flag"""
    for name, o in R.OPS.items():
        limbs = [R.s32(w) for v in o.vectors() for k in range(12) for w in v[9 * k:9 * k + 8]]
        vals = [abs(R.val([R.s32(w) for w in v[9 * k:9 * k + 9]])) for v in o.vectors() for k in range(12)]
        if name != "sx_expt":  # a power is checked on cyclotomic operands only, which cannot be chosen limb by limb
            assert R.B28 in limbs and -R.B28 in limbs, name
            assert {"one", "minus_one", "fp", "fp2", "fp6", "w^5"} <= {l.split("*")[0].split("/")[0] for l in o.labels()} or \
                name.startswith("sx_mulv"), name
        assert 100 * max(vals) > (R.IN_BOUND[name] - 2) * R.P, name  # within 0.02 p of the stated bound
        assert 2 * max(vals) > R.P, name                                 # a representative beyond the centred one
    labs = R.OPS["sx_mulv"].labels()
    assert {"unit%d%d" % (i, j) for i in range(6) for j in range(6)} <= set(labs)
    for name in ("sx_fixed_line", "sx_fixed_line_n", "sx_miller3"):
        flags = {v[-1] for v in R.OPS[name].vectors()}
        assert flags == {0, 1}, name


def test_cyclotomic_squaring_operands_load_the_even_lanes():
    """sq_cyc_sqr's even lanes multiply a_p + a_(p+3): jobs whose two coefficients have every limb 0..7 at the same
    extreme make every limb of that sum +2^29 or -2^29, in all four sign patterns; the polynomial reference gs_sqr
    is the Fp12 square on the cyclotomic operands"""
    for name in ("sx_cyc_sqr", "sx_xpow_turn"):
        o = R.OPS[name]
        seen = set()
        for lab, v in zip(o.labels(), o.vectors()):
            if lab.startswith("pairs"):
                for p in range(3):
                    for c in range(2):
                        u = [R.s32(w) for w in v[18 * p + 9 * c:18 * p + 9 * c + 8]]
                        w = [R.s32(w) for w in v[18 * (p + 3) + 9 * c:18 * (p + 3) + 9 * c + 8]]
                        assert all(abs(x + y) == 1 << 29 for x, y in zip(u, w)), (name, lab)
                        seen.add(tuple(x > 0 for x in u))
            if lab.startswith("cyclo") or lab == "one":
                a = R.rd_f12(v, 0)
                assert R.gs_sqr(a) == R._t_mul(a, a), (name, lab)
        assert len(seen) == 4, name
        assert sum(lab.startswith("cyclo") for lab in o.labels()) >= 60, name


def test_full_product_exceeds_half_p(emu_sx, table):
    """Regression for the bound dev/sx29.h's opening comment used to state: a full product of reduced operands
    (|value| <= 0.52 p) was said to come back below 0.52 p, counting twelve plain field products.  Lane 0 sums
    a_0 b_0 and five wrapped terms whose multiplicands xi b_j are up to 10 |b|: the result is bounded by 1/2 +
    102 |a| |b| / 168.9 (0.663 p), and on the 'half' jobs (every coefficient within 0.02 p of +-p/2) it does exceed
    0.52 p.  Named here: op, job, lane and the value, so that a change of the reduction shows."""
    worst = {}
    for name in ("sx_mulv", "sx_mulv24"):
        o = R.OPS[name]
        idx = [j for j, lab in enumerate(o.labels()) if lab.startswith("half")]
        assert len(idx) == 6
        for j in idx:
            v = o.vectors()[j]
            for k in range(24):  # both operands reduced
                assert 100 * abs(R.val([R.s32(w) for w in v[9 * k:9 * k + 9]])) <= 52 * R.P
            out = ctypes.create_string_buffer(R.OUT * 4)
            assert emu_sx.sxe_sx_ops(table[name][0], 1, R.pack(v), out) == 0
            got = struct.unpack("<%dI" % R.OUT, out.raw)
            R.check_job(name, o.labels()[j], o.expected()[j], got)
            for k in range(6):
                for c in range(2):
                    m = abs(R.val([R.s32(w) for w in got[18 * k + 9 * c:18 * k + 9 * c + 9]])) / R.P
                    assert m <= float(R._pb(102, "0.52", "0.52")), (name, o.labels()[j], k, c, m)
                    worst[name] = max(worst.get(name, (0,)), (m, o.labels()[j], k, c))
    print("largest full product of reduced operands:", worst)
    # sx_mulv24, job half0, lane 0, c0: 0.5520 p (lane 0 has the most wrapped terms)
    m, lab, k, c = worst["sx_mulv24"]
    assert (lab, k, c) == ("half0", 0, 0) and 0.52 < m < 0.56, worst


def test_unit_pairs_reference():
    """w^i w^j = w^((i + j) mod 6), times xi when i + j >= 6: the reference itself on the 36 pairs"""
    o = R.OPS["sx_mulv"]
    seen = 0
    for lab, want in zip(o.labels(), o.expected()):
        if lab.startswith("unit"):
            i, j = int(lab[4]), int(lab[5])
            e = [R.C.F2_ZERO] * 6
            e[(i + j) % 6] = R.C.XI if i + j >= 6 else R.C.F2_ONE
            assert list(want) == e, lab
            seen += 1
    assert seen == 36


@pytest.mark.parametrize("name", list(R.NIN))
def test_emulation_matches_reference(name, emu_sx, table):
    o = R.OPS[name]
    out = ctypes.create_string_buffer(R.N_JOBS * R.OUT * 4)
    assert emu_sx.sxe_sx_ops(table[name][0], R.N_JOBS, o.packed(), out) == 0
    R.check_op(name, struct.unpack("<%dI" % (R.N_JOBS * R.OUT), out.raw))


def test_sx_vectors_kill_mutants():
    for name, what, mutant in R.MUTANTS:
        o = R.OPS[name]
        assert any(tuple(mutant(name, v)) != e for v, e in zip(o.vectors(), o.expected())), (name, what)
    # the schoolbook product the mutants are built on is the reference when nothing is dropped
    o = R.OPS["sx_mulv"]
    assert all(tuple(R.ref("sx_mulv", v, mul=R.w_mul)) == e for v, e in zip(o.vectors()[:40], o.expected()))
    assert all(tuple(R.ref(n, v, frob=R.w_frob)) == e for n in ("sx_frob1", "sx_frob2", "sx_frob3")
               for v, e in zip(R.OPS[n].vectors()[:20], R.OPS[n].expected()))
