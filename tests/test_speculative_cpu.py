"""kr_lookup_draft (the drafting rule of greedy prompt-lookup speculation, host only) against a Python restatement of the rule."""
import numpy as np
import pytest

from krasis_amd.decode_store import lookup_draft


def rule(h, ngram_max, max_draft):
    """For g = min(ngram_max, n-1) down to 1: the largest j with j + g <= n-1 and h[j:j+g] == h[n-g:]; the first g that matches gives
    h[j+g : min(j+g+max_draft, n)].  No match: []."""
    n = len(h)
    for g in range(min(ngram_max, n - 1), 0, -1):
        for j in range(n - 1 - g, -1, -1):
            if h[j:j + g] == h[n - g:]:
                return h[j + g:min(j + g + max_draft, n)]
    return []


@pytest.mark.parametrize("alphabet", [2, 3, 5, 50])
@pytest.mark.parametrize("ngram_max", [1, 2, 3, 7])
def test_random_histories_match_the_rule(alphabet, ngram_max):
    rng = np.random.default_rng(alphabet * 100 + ngram_max)
    for trial in range(150):
        n = int(rng.integers(0, 40))
        h = [int(x) for x in rng.integers(0, alphabet, n)]
        for max_draft in (0, 1, 4, 15):
            assert lookup_draft(h, ngram_max, max_draft) == rule(h, ngram_max, max_draft), (h, ngram_max, max_draft)


def test_empty_and_single_token_histories():
    assert lookup_draft([], 3, 8) == []
    assert lookup_draft([42], 3, 8) == []
    assert lookup_draft([4, 4], 3, 8) == [4]          # g = 1: h[0] == h[1], continuation h[1:]


def test_run_of_one_token():
    h = [9] * 10
    # g = 3: the largest j with j + 3 <= 9 is 6 -> the draft is the last token alone
    assert lookup_draft(h, 3, 8) == [9] == rule(h, 3, 8)
    assert lookup_draft(h, 1, 8) == [9]


def test_continuation_overlaps_the_trailing_ngram():
    # the latest earlier occurrence of (1, 2) starts at 2; its continuation runs into the trailing n-gram itself
    h = [5, 6, 1, 2, 1, 2]
    assert lookup_draft(h, 2, 8) == [1, 2] == rule(h, 2, 8)
    h = [1, 2, 3, 1, 2, 3, 1, 2]
    assert lookup_draft(h, 3, 8) == [3, 1, 2] == rule(h, 3, 8)


def test_longest_ngram_wins_over_a_later_shorter_match():
    h = [1, 2, 3, 7, 9, 3, 8, 2, 3]
    # g = 2: (2, 3) occurs at 1 -> continuation 7, 9, ...; g = 1 alone would pick the later 3 at 5 -> 8
    assert lookup_draft(h, 2, 3) == [7, 9, 3]
    assert lookup_draft(h, 1, 3) == [8, 2, 3]


def test_max_draft_truncation():
    h = list(range(20)) + [0, 1]
    for md in range(0, 16):
        assert lookup_draft(h, 2, md) == list(range(2, 2 + md))


def test_argument_errors():
    with pytest.raises(ValueError):
        lookup_draft([1, 2, 3], 0, 4)
    with pytest.raises(ValueError):
        lookup_draft([1, 2, 3], 2, -1)
