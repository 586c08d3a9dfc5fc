"""min_match, the integer the groups entries take in place of a threshold (include/tiktoken_amd.h), against the comparison
Fingerprints.duplicate_groups makes: count / P >= threshold in float64."""
import math

import numpy as np
import pytest

from tiktoken_amd._tiktoken import min_match


def thresholds(P):
    ts = [0.0, 0.5, 0.8, 1.0, 1.0000001, -1.0, math.nan]
    for k in {0, 1, P // 3, P - 1, P}:
        ts += [np.nextafter(k / P, -1.0), k / P, np.nextafter(k / P, 2.0)]
    return ts


@pytest.mark.parametrize("P", [1, 6, 128, 256])
def test_min_match_is_the_least_count_that_passes(P):
    for t in thresholds(P):
        passes = [c for c in range(P + 1) if np.float64(c) / np.float64(P) >= np.float64(t)]  # (the helper's comparison, count by count)
        c = min_match(t, P)
        assert c == (passes[0] if passes else P + 1), (P, t)
        assert passes == list(range(c, P + 1)), (P, t, "the counts that pass are not the counts from min_match on")
