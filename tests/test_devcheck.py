"""Device primitive conformance: every arithmetic primitive of dev/fp.h,
dev/fp_wide.h, dev/fp29.h, dev/sha256.h and dev/p256.h on operands chosen here,
every result word against the big-integer references of tests/devcheck_ref.py.

The device build of this layer is largely other source than the host build
(asm carry chains and products, __builtin_addc/subc, 16-byte loads), and the
suite above it only sees the values valid proofs produce.  Two tiers run the
same vectors through the same dispatcher (csrc/tools/devcheck_ops.h):
  CPU  tests/native/devcheck_host.cpp, built plainly, with FTS_HOST64 and as
       a stand-alone ASan + UBSan program: validates vectors, packing and
       references, and the host branches;
  GPU  libftsdevcheck.so (csrc/tools/devcheck.hip): one kernel per op, one
       vector per lane, workgroups of 64 and 256 lanes with a partial last one,
       single and chained ((a o b) o a) o b variants.
Every comparison is exact.  test_vectors_kill_mutants shows that the vectors
tell plausible wrong kernels from the right one.
"""
import ctypes
import os
import struct
import subprocess

import pytest

import devcheck_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "devcheck_host.cpp")
LIB = os.path.join(ROOT, "fabric-token-sdk_amd", "zkatdlog", "_lib", "libftsdevcheck.so")
GROUPS = R.GROUPS + ["sha"]


def _build(out, extra):
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas"] + extra + [SRC, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def host_bins(tmp_path_factory):
    d = tmp_path_factory.mktemp("devcheck")
    plain = _build(str(d / "devcheck_host"), [])
    host64 = _build(str(d / "devcheck_host64"), ["-DFTS_HOST64"])  # the product's host-side 4 x 64-bit products
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    try:  # the sanitizer runtimes inside the program, where the toolchain ships them as archives
        san = _build(str(d / "devcheck_host_san"), flags + ["-static-libasan", "-static-libubsan"])
    except subprocess.CalledProcessError:
        san = _build(str(d / "devcheck_host_san"), flags)
    return plain, san, host64


@pytest.fixture(scope="module")
def table(host_bins):
    """the header's op table: name -> (index, nin, nout)"""
    out = subprocess.run([host_bins[0], "--table"], check=True, capture_output=True, text=True).stdout
    return {f[1]: (int(f[0]), int(f[2]), int(f[3])) for f in (ln.split() for ln in out.splitlines())}


@pytest.fixture(scope="module")
def stream(table):
    """every vector of every op, then the hash set, as the host program reads them"""
    recs = [struct.pack("<2I", table[name][0], len(o.vectors())) + o.packed() for name, o in R.OPS.items()]
    return b"".join(recs) + R.sha_set().record()


def split_output(raw):
    """the host program's output -> {op name: flat words}, 'sha': flat words"""
    out, pos = {}, 0
    for name, o in R.OPS.items():
        n = len(o.vectors()) * o.nout
        out[name] = struct.unpack_from("<%dI" % n, raw, pos)
        pos += 4 * n
    n = R.sha_set().n * 16
    out["sha"] = struct.unpack_from("<%dI" % n, raw, pos)
    assert pos + 4 * n == len(raw)
    return out


@pytest.fixture(scope="module")
def host_raw(host_bins, stream):
    r = subprocess.run([host_bins[0]], input=stream, capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def check_words(name, vectors, expected, got, nout):
    """every output word of every vector; returns the number of vectors compared"""
    assert len(got) == len(vectors) * nout, name
    bad = [j for j in range(len(vectors)) if tuple(got[j * nout:(j + 1) * nout]) != tuple(expected[j])]
    assert not bad, "%s: %d of %d vectors differ; first: in %s got %s want %s" % (
        name, len(bad), len(vectors), [hex(w) for w in vectors[bad[0]][:18]],
        [hex(w) for w in got[bad[0] * nout:(bad[0] + 1) * nout]], [hex(w) for w in expected[bad[0]]])
    return len(vectors) - len(bad)


def check_op(name, got):
    o = R.OPS[name]
    vs = o.vectors()
    assert check_words(name, vs, o.expected(), got, o.nout) == len(vs)
    checked = [R.f29_check_bounds(name, v, got[j * o.nout:(j + 1) * o.nout]) for j, v in enumerate(vs)]
    assert all(c is not False for c in checked), (name, "documented bound or congruence", checked.index(False))
    if name in ("f29_mul", "f29_norm", "f29_reduce", "f29_sqr", "f29_mul_c", "f29_sqr_c"):
        assert all(c is True for c in checked)


def check_sha(got):
    s = R.sha_set()
    seglists = [tuple(x for seg in s.segs[s.first[j]:s.first[j + 1]] for x in seg) for j in range(s.n)]
    assert check_words("sha", seglists, s.expected(), got, 16) == s.n


def check_group(group, outputs):
    if group == "sha":
        return check_sha(outputs["sha"])
    names = [n for n, o in R.OPS.items() if o.group == group]
    assert names
    for n in names:
        check_op(n, outputs[n])
    if group == "f29":  # the two forms of the product give the same limbs
        assert outputs["f29_mul"] == outputs["f29_mul_c"] and outputs["f29_sqr"] == outputs["f29_sqr_c"]


# ------------------------------------------------------------------ CPU tier
def test_every_op_has_vectors(table):
    """an op added to the header's table without vectors and a reference fails here"""
    assert set(table) == set(R.OPS), set(table) ^ set(R.OPS)
    assert sorted(i for i, _, _ in table.values()) == list(range(len(table)))
    for name, (_, nin, nout) in table.items():
        o = R.OPS[name]
        assert (o.nin, o.nout) == (nin, nout), name
        assert o.group in R.GROUPS and len(o.vectors()) > 0 and len(o.expected()) == len(o.vectors()), name
        assert len(o.vectors()) % 64 and len(o.vectors()) % 256, name  # a partial last workgroup at both sizes
    assert table["w2_sum"][1] == R.W2_IN
    s = R.sha_set()
    assert s.n % 256 and {len(m) for m in s.msgs} == set(R.SHA_LENGTHS)
    for want in ["one@%d" % k for k in range(16)] + ["split+empty", "split3", "blocks+tail", "partial+aligned64"]:
        assert want in s.labels
    for j, lab in enumerate(s.labels):  # the placements are what their labels say
        segs = s.segs[s.first[j]:s.first[j + 1]]
        if lab == "partial+aligned64":
            assert 0 < segs[0][1] < 64 and segs[1][0] % 16 == 0 and segs[1][1] >= 64 and s.fast_blocks(j) == 0
        if lab == "blocks+tail":
            assert segs[0][0] % 16 == 0 and segs[0][1] % 64 == 0 and s.fast_blocks(j) >= segs[0][1] // 64 > 0


@pytest.mark.parametrize("group", GROUPS)
def test_host_matches_reference(group, host_raw):
    check_group(group, split_output(host_raw))


def test_host_clean_under_sanitizers(host_bins, stream, host_raw):
    """the same vectors through the stand-alone ASan + UBSan build: no report (a signed column overflow of
    dev/fp29.h at a documented bound would be one), and the same words"""
    r = subprocess.run([host_bins[1]], input=stream, capture_output=True)
    assert r.returncode == 0, r.stderr[-3000:].decode(errors="replace")
    assert r.stdout == host_raw


def test_host64_products_give_the_same_words(host_bins, stream, host_raw):
    """FTS_HOST64 (build.py's define: operator* in 4 x 64-bit limbs on the host) against the 32-bit CIOS"""
    r = subprocess.run([host_bins[2]], input=stream, capture_output=True)
    assert r.returncode == 0 and r.stdout == host_raw


def test_vectors_kill_mutants():
    for name, what, mutant in R.MUTANTS:
        o = R.OPS[name]
        assert any(tuple(mutant(v)) != e for v, e in zip(o.vectors(), o.expected())), (name, what)
    for name, what, mutant in R.EQUIVALENT_MUTANTS:  # no output shows it: see devcheck_ref.py
        o = R.OPS[name]
        assert all(tuple(mutant(v)) == e for v, e in zip(o.vectors(), o.expected())), (name, what)
    s = R.sha_set()
    want = s.expected()
    for what, mutant in R.SHA_MUTANTS:
        assert any(tuple(mutant(s, j)) != want[j] for j in range(s.n)), what
    # the limb-for-limb model the f29 mutant is built on is the reference when nothing is flipped
    o = R.OPS["f29_mul"]
    assert all(R.f29_mul_model([R.s32(w) for w in v[:9]], [R.s32(w) for w in v[9:]]) == e
               for v, e in zip(o.vectors(), o.expected()))


# ------------------------------------------------------------------ GPU tier
@pytest.fixture(scope="module")
def devlib(table):
    lib = ctypes.CDLL(LIB)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.ftz_devcheck_info.argtypes = [ctypes.c_int, ctypes.c_char_p, u32p, u32p]
    lib.ftz_devcheck.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p,
                                 ctypes.c_char_p]
    lib.ftz_devcheck_sha.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32,
                                     ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    name, nin, nout = ctypes.create_string_buffer(32), ctypes.c_uint32(), ctypes.c_uint32()
    count = lib.ftz_devcheck_info(-1, name, nin, nout)
    got = {}
    for i in range(count):
        lib.ftz_devcheck_info(i, name, nin, nout)
        got[name.value.decode()] = (i, nin.value, nout.value)
    assert got == table  # the library and the host program were built from the same table
    return lib


def split_lanes(name, raw, n, block, nout):
    """the harness's output buffer -> the n lanes' words, after checking the idle lanes' sentinel"""
    lanes = -(-n // block) * block
    assert n % block and len(raw) == lanes * nout * 4
    got = struct.unpack("<%dI" % (lanes * nout), raw)
    assert all(w == R.SENTINEL for w in got[n * nout:]), name + ": a lane past n wrote"
    return got[:n * nout]


@pytest.mark.gpu
@pytest.mark.parametrize("block", [64, 256])
@pytest.mark.parametrize("group", GROUPS)
def test_device_matches_reference(group, block, devlib, table):
    outputs = {}
    if group == "sha":
        s = R.sha_set()
        out = ctypes.create_string_buffer(-(-s.n // block) * block * 64)
        rc = devlib.ftz_devcheck_sha(0, s.n, block, bytes(s.arena), len(s.arena), struct.pack("<%dI" % len(s.first), *s.first),
                                     b"".join(struct.pack("<2I", *x) for x in s.segs), out)
        assert rc == 0
        outputs["sha"] = split_lanes("sha", out.raw, s.n, block, 16)
    for name, o in R.OPS.items():
        if o.group != group:
            continue
        n = len(o.vectors())
        out = ctypes.create_string_buffer(-(-n // block) * block * o.nout * 4)
        rc = devlib.ftz_devcheck(0, table[name][0], n, block, o.packed(), out)
        assert rc == 0, (name, rc)
        outputs[name] = split_lanes(name, out.raw, n, block, o.nout)
    check_group(group, outputs)
