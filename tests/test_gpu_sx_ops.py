"""The sextet pairing routines of dev/sx29.h on the device, op by op, against
the Fp12 references of tests/sx_ref.py (GPU tier of tests/test_sx_ops.py).

libftsdevcheck.so (csrc/tools/devcheck.hip, ftz_devcheck_sx) runs one kernel per
op of csrc/dev/devcheck_sx.h with the runtime's launch shape and prologue: 64
lanes per workgroup, ten sextets and the ghost lanes 60..63, the production LDS
regions and barrier.  The words are the ones the host emulation passed on, so a
failure here names what only the device has: the LDS exchange, a barrier, the
ghost lanes, a compiled lane-role select -- and the op, the job and the lane.
  - every lane's value mod p equals the big-integer reference (exact);
  - limbs 0..7 are balanced and the value is within the routine's stated bound;
  - the result buffer covers every sextet of every workgroup: the sextets past n
    leave their sentinel alone;
  - n = 153 (sixteen workgroups, the last of three jobs), and 1, 10, 11 and 23
    jobs: one sextet, a full wave, a second workgroup of one job, a partial third.
sx_miller3 and sx_xpow_turn chain routines with nothing republished in between:
a missing trailing barrier corrupts the next routine's LDS reads there.
Each op is launched once per job count; nothing is retried.
"""
import ctypes
import os
import struct

import pytest

import sx_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fabric-token-sdk_amd", "zkatdlog", "_lib", "libftsdevcheck.so")


@pytest.fixture(scope="module")
def devlib():
    lib = ctypes.CDLL(LIB)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.ftz_devcheck_sx_info.argtypes = [ctypes.c_int, ctypes.c_char_p, u32p, u32p, u32p, u32p]
    lib.ftz_devcheck_sx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p]
    return lib


@pytest.fixture(scope="module")
def table(devlib):
    name = ctypes.create_string_buffer(32)
    v = [ctypes.c_uint32() for _ in range(4)]
    out = {}
    for i in range(devlib.ftz_devcheck_sx_info(-1, name, *v)):
        devlib.ftz_devcheck_sx_info(i, name, *v)
        out[name.value.decode()] = (i,) + tuple(x.value for x in v)
    # the library was built from the table the vectors were written for
    assert {k: t[1:] for k, t in out.items()} == {k: (R.NIN[k], R.OUT) + R.LAYOUT[k] for k in R.NIN}
    return out


def run_op(devlib, table, name, n):
    """the op on its first n jobs: the n jobs' words, after checking that no sextet past n wrote"""
    slots = -(-n // 10) * 10
    out = ctypes.create_string_buffer(slots * R.OUT * 4)
    rc = devlib.ftz_devcheck_sx(0, table[name][0], n, R.OPS[name].packed(n), out)
    assert rc == 0, (name, n, rc)
    got = struct.unpack("<%dI" % (slots * R.OUT), out.raw)
    assert all(w == R.SENTINEL for w in got[n * R.OUT:]), "%s n=%d: a sextet past n wrote" % (name, n)
    return got[:n * R.OUT]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.NIN))
def test_device_sx_op_matches_reference(name, devlib, table):
    R.check_op(name, run_op(devlib, table, name, R.N_JOBS))


@pytest.mark.gpu
@pytest.mark.parametrize("n", R.JOB_COUNTS)
def test_device_sx_job_counts(n, devlib, table):
    for name in R.NIN:
        R.check_op(name, run_op(devlib, table, name, n), n)
