"""The pairing stage on the device as the runtime launches it, over jobs whose
GT value is known by bilinearity (tests/pair_ref.py, csrc/tools/devpair.hip).

libftsdevpair.so runs k_qlines, the G2 stage, then k_miller or k_miller_n --
chosen here, so the unnormalised fallback k_miller runs although no public
parameters of the suite have a fixed line with r0 = 0 -- and launch_fexp itself,
exact or Fuentes-Castaneda, writing GT bytes or the unity byte; a second entry
does the same for k_miller_f3 with three fixed G2 arguments.  Per job count (1,
10, 11 and 21 jobs: one sextet, a full wave, a second and a third workgroup of a
single job) and per combination:
  - every job's 384 GT bytes equal the reference (so k_miller and k_miller_n
    agree byte for byte): random jobs, P1, R or t' at infinity, all at once
    (GT = 1), a product that cancels to one with no point at infinity and its
    neighbour with the exponent off by one;
  - the unity kernels' bytes: one for the cancelling products and the all-
    infinity jobs, zero for the rest, also for a job alone in its workgroup
    and for the sextet the ghost lanes shadow;
  - no arena byte outside a job's 384 changes, no unity byte, arena place or
    F12 value of a sextet past n, and no park entry of a ghost lane.
A single job is launched three times, on a cancelling product, its neighbour
with exponent one and a random job, so the one-sextet launch sees both unity
bytes and non-trivial GT bytes.  Each combination is one call; nothing is retried.
"""
import ctypes
import os

import pytest

import pair_ref as PR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fabric-token-sdk_amd", "zkatdlog", "_lib", "libftsdevpair.so")


@pytest.fixture(scope="module")
def devlib():
    lib = ctypes.CDLL(LIB)
    cp, u32 = ctypes.c_char_p, ctypes.c_uint32
    lib.ftz_devcheck_pair_jobs.argtypes = [ctypes.c_int, u32, ctypes.c_int, ctypes.c_int, ctypes.c_int, cp, cp, cp, cp,
                                           u32, cp, u32, cp, cp, cp, ctypes.POINTER(u32)]
    lib.ftz_devcheck_pair3_jobs.argtypes = [ctypes.c_int, u32, ctypes.c_int, ctypes.c_int, cp, cp, cp, cp,
                                            ctypes.POINTER(u32)]
    return lib


def buffers(n):
    slots = -(-n // 10) * 10
    return ctypes.create_string_buffer(PR.GAP + slots * PR.STRIDE), ctypes.create_string_buffer(slots), ctypes.c_uint32(99)


@pytest.mark.parametrize("n", PR.JOB_COUNTS)
@pytest.mark.parametrize("miller", [0, 1], ids=["k_miller", "k_miller_n"])
def test_two_pair_stage_matches_bilinearity(devlib, miller, n):
    jobs = PR.pair_jobs()
    for start, exact, unity in ((s, e, u) for s in PR.STARTS.get(n, (0,)) for e in (1, 0) for u in (0, 1)):
        a = jobs.packed(n, start)
        arena, ok, guard = buffers(n)
        rc = devlib.ftz_devcheck_pair_jobs(0, n, miller, exact, unity, a["q"], a["p1"], a["jobs"], a["bases"],
                                           a["n_scal"], a["scal"], a["n_pts"], a["pts"], arena, ok,
                                           ctypes.byref(guard))
        what = "%s n=%d from job %d %s %s" % ("k_miller_n" if miller else "k_miller", n, start,
                                              "exact" if exact else "fuentes", "unity" if unity else "bytes")
        assert rc == 0, (what, rc)
        PR.check_outputs(jobs, n, bool(exact), bool(unity), arena.raw, ok.raw, guard.value, what, start)


@pytest.mark.parametrize("n", PR.JOB_COUNTS)
def test_three_pair_stage_matches_bilinearity(devlib, n):
    jobs = PR.pair3_jobs()
    for start, exact, unity in ((s, e, u) for s in PR.STARTS.get(n, (0,)) for e in (1, 0) for u in (0, 1)):
        a = jobs.packed(n, start)
        arena, ok, guard = buffers(n)
        rc = devlib.ftz_devcheck_pair3_jobs(0, n, exact, unity, a["q3"], a["pts3"], arena, ok, ctypes.byref(guard))
        what = "k_miller_f3 n=%d from job %d %s %s" % (n, start, "exact" if exact else "fuentes",
                                                       "unity" if unity else "bytes")
        assert rc == 0, (what, rc)
        PR.check_outputs(jobs, n, bool(exact), bool(unity), arena.raw, ok.raw, guard.value, what, start)
