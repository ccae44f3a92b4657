"""Host side of the eval stage, no GPU: `evl.metric._ranked_topk` decides which expert ids the metric kernels see for every prediction
matrix and `.pred` file, so it is compared here with the metric oracle's `ranked_list` (trec_eval's ordering) on scores without ties, and
with the order the module's docstring promises (ascending expert id) where scores are equal.  Also pins `skill_coverage_ranked`, the
oracle entry the device tests feed ranked lists to, on the reference-shaped `skill_coverage`."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import metric_oracle as MO
from opentf_amd.evl.metric import _ranked_topk


def _distinct_scores(rng, n, M, dtype=np.float32):
    """[n, M] strictly positive scores in (0.1, 1), distinct within a row by construction (a permuted grid), exact in f32"""
    grid = (0.1 + 0.9 * (np.arange(M, dtype=np.float64) + 1.0) / (M + 1.0)).astype(dtype)
    assert len(np.unique(grid)) == M
    return np.stack([grid[rng.permutation(M)] for _ in range(n)])


def _sparse_case(rng, n, M, counts, shuffle):
    """CSR [n, M] with counts[i] stored, distinct, positive scores in row i; `shuffle`: stored order inside a row is random (unsorted indices)"""
    dense = _distinct_scores(rng, n, M)
    indptr, indices, data = [0], [], []
    for i in range(n):
        cols = rng.choice(M, counts[i], replace=False)
        cols = cols if shuffle else np.sort(cols)
        indices.append(cols); data.append(dense[i, cols]); indptr.append(indptr[-1] + counts[i])
    S = sp.csr_matrix((np.concatenate(data).astype(np.float32), np.concatenate(indices).astype(np.int32), np.array(indptr, np.int64)), shape=(n, M))
    if not shuffle:
        S.sort_indices()
    return S


def _oracle_ranks(D, k):
    return np.stack([MO.ranked_list(D[i], k) for i in range(D.shape[0])]).astype(np.int32)


@pytest.mark.parametrize("n,M,k", [(7, 50, 10), (3, 50, 1), (3, 50, 50), (1, 1, 1), (5, 1000, 128), (2, 300, 299)])
def test_ranked_topk_dense_equals_the_oracle_ranking(n, M, k):
    rng = np.random.default_rng(1000 * M + k)
    for dtype in (np.float32, np.float64):
        D = _distinct_scores(rng, n, M, dtype)
        got = _ranked_topk(D, k)
        assert got.dtype == np.int32 and got.shape == (n, k) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, _oracle_ranks(D.astype(np.float64), k))


@pytest.mark.parametrize("shuffle", [False, True], ids=["sorted_indices", "unsorted_indices"])
@pytest.mark.parametrize("M,k", [(40, 8), (40, 1), (40, 40), (500, 64)])
def test_ranked_topk_sparse_equals_the_oracle_ranking(M, k, shuffle):
    """rows that store 0, 1, fewer than k, exactly k, more than k and all M entries, in one matrix"""
    rng = np.random.default_rng(M + 7 * k + shuffle)
    counts = sorted({0, 1, max(k - 1, 0), k, min(k + 1, M), min(2 * k + 3, M), M})
    counts = counts + counts[::-1]          # each kind twice, so that a short row also follows a long one
    S = _sparse_case(rng, len(counts), M, counts, shuffle)
    unsorted_rows = sum(bool((np.diff(S.indices[S.indptr[i]:S.indptr[i + 1]]) < 0).any()) for i in range(len(counts)))
    assert (unsorted_rows >= 4) if shuffle else (unsorted_rows == 0)
    before = (S.indptr.copy(), S.indices.copy(), S.data.copy())
    got = _ranked_topk(S, k)
    assert got.dtype == np.int32 and got.shape == (len(counts), k)
    assert np.array_equal(got, _oracle_ranks(MO.tiebreak_free_dense(S), k))
    for a, b in zip(before, (S.indptr, S.indices, S.data)):
        assert np.array_equal(a, b)         # the caller's matrix is not reordered
    # other sparse formats and a float64 matrix go the same way
    assert np.array_equal(_ranked_topk(S.tocoo(), k), got) and np.array_equal(_ranked_topk(S.astype(np.float64).tocsc(), k), got)


def test_ranked_topk_orders_equal_scores_by_ascending_id():
    """f32 scores with explicit tie groups, one of them straddling the k-th place: ascending expert id inside a group (the module's docstring;
    trec_eval itself would order a tie by descending document NAME, which is why the device tests feed ranked lists, not scores)"""
    M, k = 30, 12
    row = np.full(M, 0.25, np.float32)
    row[[17, 3, 22]] = 0.9            # a tie group at the top
    row[[5]] = 0.8
    row[[29, 0, 11, 12]] = 0.5        # a tie group in the middle
    # the remaining 22 experts tie at 0.25 and the k-th place falls among them
    rest = [c for c in range(M) if c not in (17, 3, 22, 5, 29, 0, 11, 12)]
    expect = np.array([3, 17, 22, 5, 0, 11, 12, 29] + rest[:4], dtype=np.int32)
    assert np.array_equal(_ranked_topk(row[None], k)[0], expect)
    assert np.array_equal(_ranked_topk(np.stack([row, row[::-1]]), k)[1], np.lexsort((np.arange(M), -row[::-1].astype(np.float64)))[:k])
    # the same row stored sparsely (every entry, shuffled), and with only the 8 leaders stored: the unstored experts tie at 0
    perm = np.random.default_rng(0).permutation(M)
    S = sp.csr_matrix((row[perm], perm.astype(np.int32), np.array([0, M])), shape=(1, M))
    assert np.array_equal(_ranked_topk(S, k)[0], expect)
    lead = np.array([29, 22, 12, 17, 11, 0, 5, 3], dtype=np.int32)
    S8 = sp.csr_matrix((row[lead], lead, np.array([0, 8])), shape=(1, M))
    assert np.array_equal(_ranked_topk(S8, k)[0], np.array([3, 17, 22, 5, 0, 11, 12, 29, 1, 2, 4, 6], dtype=np.int32))


def test_ranked_topk_dense_and_sparse_routes_agree_on_random_small_cases():
    """200 random small cases: a sparse matrix with positive stored scores and its dense form (zeros where nothing is stored) rank alike for
    every k, rows shorter than k included - the dense route's stable argsort puts the zeros in id order, the sparse route completes by id."""
    rng = np.random.default_rng(2024)
    short_rows = 0
    for case in range(200):
        n, M = int(rng.integers(1, 7)), int(rng.integers(1, 41))
        k = int(rng.integers(1, M + 1))
        counts = rng.integers(0, M + 1, n)
        S = _sparse_case(rng, n, M, counts, shuffle=bool(case % 2))
        short_rows += int((counts < k).sum())
        a, b = _ranked_topk(S, k), _ranked_topk(S.toarray(), k)
        assert np.array_equal(a, b), (case, n, M, k, counts)
        assert all(len(set(r.tolist())) == k for r in a)            # a ranking never names an expert twice
    assert short_rows > 100                                         # the completion path was really exercised


def test_skill_coverage_ranked_equals_the_reference_shaped_oracle():
    """`skill_coverage_ranked` (a ranking in, for the device tests) against `skill_coverage` (scores in, the reference's own code shape) on
    scores that reproduce the ranking: score = -position."""
    rng = np.random.default_rng(5)
    E, S = 60, 90
    nnz = rng.integers(0, 12, E); nnz[[0, 7]] = 0
    cip = np.concatenate([[0], np.cumsum(nnz)]).astype(np.int64)
    cix = np.concatenate([np.sort(rng.choice(S, c, replace=False)) for c in nnz]).astype(np.int32)
    for trial in range(40):
        ranked = rng.permutation(E)
        scores = np.empty(E); scores[ranked] = -np.arange(E, dtype=np.float64)
        req = rng.choice(S, int(rng.integers(1, 30)), replace=False)
        cut = (1, 2, 5, 10, 59, 60)
        assert MO.skill_coverage_ranked(ranked, req, cip, cix, cut) == MO.skill_coverage(scores, req, cip, cix, cut)
    # a cutoff above the list takes the whole list; an instance without a required skill is an error, as in the reference
    assert MO.skill_coverage_ranked(ranked[:10], req, cip, cix, (10, 100))["skill_coverage_100"] == MO.skill_coverage_ranked(ranked[:10], req, cip, cix, (10,))["skill_coverage_10"]
    with pytest.raises(ZeroDivisionError):
        MO.skill_coverage_ranked(ranked, np.array([], np.int32), cip, cix, (2,))
