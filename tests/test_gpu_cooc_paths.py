"""Member-skill co-occurrence (`ntf_skill_cooccurrence`, opentf_amd/csrc/ntf_cooc.hip) on a real MI355X on the branches tests/test_gpu_cooc.py does not
reach: the scan's second and third strip of block sums, the wave sort at every padded size and at SORT_MAX, the histogram kernel's pass edges, its
wrapped counts and its second and third round on a scratch row, rows with work and nothing to store, and the entry's refusals.  The cases and what
each of them reaches are tests/cooc_cases.py's, asserted without a device by tests/test_cooc_host.py; the reference is oracle/cooc_oracle.py (pinned
there on the reference's own expression for every case).  Integer work: every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import cooc_cases as CC

pytestmark = pytest.mark.gpu


def _run(name, skipped=True, return_ms=False):
    from opentf_amd.cmn.team import skill_cooccurrence
    m_ip, m_ix, s_ip, s_ix, n, M, S, skip = CC.case(name)
    return skill_cooccurrence((m_ip, m_ix, (n, M)), (s_ip, s_ix, (n, S)), skip if skipped else None, return_ms=return_ms)


def _same(got, exp, M, S):
    assert got.shape == (M, S) and got.dtype == np.uint8 and got.data.dtype == np.uint8
    assert np.array_equal(got.indptr, exp[0]), f"indptr differs first at member {int(np.nonzero(got.indptr != exp[0])[0][0]) - 1}"
    assert np.array_equal(got.indices, exp[1]) and np.array_equal(got.data, exp[2])
    rows = np.repeat(np.arange(M), np.diff(got.indptr))
    assert (np.diff(got.indices)[np.diff(rows) == 0] > 0).all()                # ascending inside every row
    assert got.has_sorted_indices


@pytest.mark.parametrize("skipped", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("name", CC.NAMES)
def test_cooc_bitexact_vs_oracle_on_every_path(name, skipped):
    c = CC.case(name)
    got, ms = _run(name, skipped, return_ms=True)
    p = CC.profile(c, skipped)
    print(f"\ncooc_paths {name} {'skip' if skipped else 'noskip'}: sort rows {p['sort_rows']}, hist rows {p['hist_rows']}, strips {p['strips']}, rounds {p['rounds']}, "
          f"nnz {got.nnz}, device {ms:.3f} ms")
    _same(got, CC.expected(name, skipped), c[5], c[6])


def test_hist_rounds_is_the_same_bytes_on_every_call_and_after_a_wider_call():
    """which long rows share a scratch row of the histogram kernel depends on the order of the sort kernel's atomics: three calls, then one after a
    call that left other sizes behind in the allocator"""
    c, exp = CC.case("hist_rounds"), CC.expected("hist_rounds")
    first = _run("hist_rounds")
    _same(first, exp, c[5], c[6])
    for _ in range(2):
        again = _run("hist_rounds")
        assert again.indptr.tobytes() == first.indptr.tobytes() and again.indices.tobytes() == first.indices.tobytes() and again.data.tobytes() == first.data.tobytes()
    w = CC.case("scan_wide-263169")
    _same(_run("scan_wide-263169"), CC.expected("scan_wide-263169"), w[5], w[6])
    fourth = _run("hist_rounds")
    assert fourth.indptr.tobytes() == first.indptr.tobytes() and fourth.indices.tobytes() == first.indices.tobytes() and fourth.data.tobytes() == first.data.tobytes()


# ---------------------------------------------------------------- refusals, through the raw ABI
SENTINEL = 0x5EED


def _raw(c, out=True, **over):
    """ntf_skill_cooccurrence on case c with arguments replaced by name; a replacement of None is a null pointer -> (rc, *out, *nnz_out)"""
    from opentf_amd import libntf
    m_ip, m_ix, s_ip, s_ix, n, M, S, skip = c
    a = dict(n_teams=n, n_members=M, n_skills=S, m_indptr=m_ip, m_indices=m_ix, s_indptr=s_ip, s_indices=s_ix, skip_rows=skip, n_skip=len(skip))
    a.update(over)
    keep = [None if a[k] is None else np.ascontiguousarray(a[k], dt) for k, dt in (("m_indptr", np.int64), ("m_indices", np.int32), ("s_indptr", np.int64),
                                                                                 ("s_indices", np.int32), ("skip_rows", np.int64))]
    ptr = [None if v is None or not v.size else v.ctypes.data_as(C.c_void_p) for v in keep]
    h, nnz = C.c_void_p(SENTINEL), C.c_int64(-7)
    rc = libntf.lib().ntf_skill_cooccurrence(0, a["n_teams"], a["n_members"], a["n_skills"], ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], a["n_skip"],
                                             C.byref(h) if out else None, C.byref(nnz))
    return rc, h.value, nnz.value


def _with(a, pos, value):
    b = np.array(a); b[pos] = value
    return b


def test_refused_calls_leave_the_outputs_alone_and_the_next_call_is_right():
    from opentf_amd import libntf
    L = libntf.lib()
    name = "degenerate-skip_repeated"
    c = CC.case(name)
    m_ip, m_ix, s_ip, s_ix, n, M, S, skip = c
    assert len(m_ix) and len(s_ix) and len(skip)
    refused = {"n_teams 0": dict(n_teams=0), "n_teams -1": dict(n_teams=-1), "n_members 0": dict(n_members=0), "n_members -3": dict(n_members=-3),
               "n_skills 0": dict(n_skills=0), "n_skills -1": dict(n_skills=-1), "null m_indptr": dict(m_indptr=None), "null s_indptr": dict(s_indptr=None),
               "null m_indices with non-zeros": dict(m_indices=None), "null s_indices with non-zeros": dict(s_indices=None),
               "member -1": dict(m_indices=_with(m_ix, 4, -1)), "member = n_members": dict(m_indices=_with(m_ix, len(m_ix) - 1, M)),
               "skill = n_skills": dict(s_indices=_with(s_ix, 0, S)), "skill -1": dict(s_indices=_with(s_ix, len(s_ix) - 1, -1)),
               "skip -1": dict(skip_rows=_with(skip, 1, -1)), "skip = n_teams": dict(skip_rows=_with(skip, len(skip) - 1, n)),
               "negative n_skip": dict(n_skip=-1), "n_skip > 0 with a null list": dict(skip_rows=None)}
    for why, over in refused.items():
        rc, h, nnz = _raw(c, **over)
        assert rc == libntf.NTF_EINVAL, why
        assert h is None, f"{why}: *out is not NULL"
        assert nnz == -7, f"{why}: *nnz_out was written"
    rc, h, nnz = _raw(c, out=False)
    assert rc == libntf.NTF_EINVAL and nnz == -7
    assert L.ntf_csr_result_fetch(None, np.zeros(M + 1, np.int64).ctypes.data_as(C.c_void_p), None, None, None) == libntf.NTF_EINVAL
    L.ntf_csr_result_free(None)
    # a valid call right after: through the raw ABI, then the wrapper
    exp = CC.expected(name)
    rc, h, nnz = _raw(c)
    assert rc == 0 and h not in (None, SENTINEL) and nnz == len(exp[1])
    try:
        assert L.ntf_csr_result_fetch(h, None, None, None, None) == libntf.NTF_EINVAL            # no indptr to write to
        indptr, indices, data, ms = np.full(M + 1, -1, np.int64), np.full(nnz, -1, np.int32), np.zeros(nnz, np.uint8), C.c_double(-1)
        assert L.ntf_csr_result_fetch(h, indptr.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p), data.ctypes.data_as(C.c_void_p), C.byref(ms)) == 0
    finally:
        L.ntf_csr_result_free(h)
    assert np.array_equal(indptr, exp[0]) and np.array_equal(indices, exp[1]) and np.array_equal(data, exp[2]) and ms.value >= 0
    _same(_run(name), exp, M, S)
