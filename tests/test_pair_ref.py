"""The bilinearity reference of tests/pair_ref.py against the project's own
pairing code on the CPU, before tests/test_gpu_pair_stage.py relies on it.

tests/native/sx_emu.cpp sxe_g2lines29 is the pair stage of one job on the
host: t' = sum s_f B_f and its evaluated lines at R, the carry-free Miller
f-chain sq_miller_f with the fixed Q's lines at P1, the exact final
exponentiation.  Its GT bytes must be those of g^(a q + r t): that fixes the
order of the pairs and that nothing is negated.  The oracle's own pairing
product of the same points must agree too.
"""
import ctypes
import random

from conftest import build_emu

import pair_ref as PR
from ftsoracle import bn254 as C


def test_bilinearity_reference_matches_host_pair_stage():
    sx = ctypes.CDLL(build_emu())
    rng = random.Random("pair-ref")
    a, r, q = (rng.randrange(1, C.R) for _ in range(3))
    b = [rng.randrange(1, C.R) for _ in range(3)]
    s = [rng.randrange(1, C.R) for _ in range(3)]
    t = sum(x * y for x, y in zip(s, b)) % C.R
    P1, Rp, Q = PR.g1_of(a), PR.g1_of(r), C.g2_mul(C.G2_GEN, q)
    bases = b"".join(C.g2_bytes(C.g2_mul(C.G2_GEN, x)) for x in b)
    gt = (ctypes.c_uint8 * 384)()
    assert sx.sxe_g2lines29(bases, C.g1_bytes(Rp), b"".join(k.to_bytes(32, "big") for k in s), C.g1_bytes(P1),
                            C.g2_bytes(Q), gt) == 0
    want = PR.gt_bytes_of((a * q + r * t) % C.R)
    assert bytes(gt) == want
    tp = C.g2_mul(C.G2_GEN, t)
    assert C.gt_bytes(C.final_exp(C.miller_loop([(P1, Q), (Rp, tp)]), C.FE_EXACT)) == want
    assert C.gt_bytes(C.final_exp(C.miller_loop([(P1, Q), (Rp, tp)]), C.FE_FUENTES)) == \
        PR.gt_bytes_of((a * q + r * t) % C.R, False)


def test_job_sets_hold_their_cases():
    for jobs, kinds in ((PR.pair_jobs(), {"random", "p1_inf", "r_inf", "t_inf", "all_inf", "cancel", "near"}),
                        (PR.pair3_jobs(), {"random", "c_inf", "all_inf", "cancel", "near"})):
        assert kinds <= {j[0] for j in jobs.jobs}
        for j, job in enumerate(jobs.jobs):
            assert jobs.unity(j) == (1 if job[0] in ("cancel", "all_inf", "p1_r_inf") else 0), (j, job[0])
        # a unity job alone in its workgroup at n = 1, 11 and 21 is covered by both values somewhere
        assert [jobs.unity(j) for j in (0, 9, 10, 20)] == [1, 1, 1, 0]
        for n in PR.JOB_COUNTS:  # both unity bytes at every job count; a single job from three starts
            assert {jobs.unity(s + j) for s in PR.STARTS.get(n, (0,)) for j in range(n)} == {0, 1}
        assert [jobs.jobs[s][0] for s in PR.STARTS[1]] == ["cancel", "near", "random"]
        assert all(jobs.exponent(j) == 1 for j, job in enumerate(jobs.jobs) if job[0] == "near")
    pj = PR.pair_jobs()
    for j, (kind, a, r, nfix, s, e) in enumerate(pj.jobs):
        if kind in ("cancel", "near"):  # no point at infinity
            assert pj.p1[j] is not None and pj.pts[j] is not None and any(pj.scal[x] for x in s[:nfix])
    assert PR.gt_bytes_of(0) == C.gt_bytes(C.F12_ONE) == PR.gt_bytes_of(0, False)
