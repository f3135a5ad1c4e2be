"""sq_rng_table_cover (include/squigly_host.h): how many seeds the table of generator words holds for a frame under a budget.

The generator of sample k of pixel (y, x) of a frame of w rows and h columns is mkTFGen (samples * (x + y * w) + k)
(src/Lib.hs:85-86), so the seeds a frame uses end at samples * ((w - 1) * w + h): that is w * h * samples for a square frame
only.  The headline frame has more rows than columns (w = 1920, h = 1080) and its last seed base is 1079 + 1919 * 1920, so a
table of w * h * samples entries would hold the seed rows of its first 1080 image rows and no other; the cover is therefore
counted from the rule itself.  Everything here is host arithmetic: no GPU."""
import pytest

MB = 1 << 20
DEFAULT_MB = 24576
HEADLINE = (1920, 1080, 256)          # rows, columns, samples (bench.py: CONFIGS["c2"])


def span(w, h, samples):
    """One past the largest seed of the frame, by the reference's rule, in Python's unbounded integers."""
    return samples * ((h - 1) + (w - 1) * w) + samples


@pytest.fixture(scope="module")
def cover(sqt):
    return sqt.lib().sq_rng_table_cover


def test_headline_frame_is_covered_by_the_default(cover):
    w, h, n = HEADLINE
    want = span(w, h, n)
    assert want == 256 * 3685560 == 943503360                      # 11.3 GB at 12 bytes
    assert want >= w * h * n                                        # never fewer than one entry per sample of the frame
    assert cover(w, h, n, DEFAULT_MB * MB) == want
    # every pixel's seed row [rix, rix + samples) lies in it: the corners and the last pixel of the first 1080 rows
    for y, x in ((0, 0), (0, h - 1), (w - 1, 0), (w - 1, h - 1), (1079, h - 1), (1080, 0)):
        assert n * (x + y * w) + n <= cover(w, h, n, DEFAULT_MB * MB)
    assert cover(w, h, 512, DEFAULT_MB * MB) == span(w, h, 512)     # the C3 stand-in (22.6 GB) fits the default too


def test_square_and_wide_frames(cover):
    assert cover(64, 64, 4, DEFAULT_MB * MB) == 64 * 64 * 4
    assert cover(40, 72, 3, DEFAULT_MB * MB) == span(40, 72, 3) == 3 * (39 * 40 + 72)   # more columns than rows: rows share seeds
    assert cover(1, 5, 7, DEFAULT_MB * MB) == 35 and cover(5, 1, 7, DEFAULT_MB * MB) == 7 * 21


def test_frame_over_the_budget_gets_a_prefix(cover):
    w, h, n = 3840, 2160, 1024                                      # the C4 frame: 181 GB of seeds
    assert span(w, h, n) * 12 > DEFAULT_MB * MB
    assert cover(w, h, n, DEFAULT_MB * MB) == DEFAULT_MB * MB // 12 == 2 ** 31
    assert cover(*HEADLINE, 100 * MB) == 100 * MB // 12             # rounded down to whole entries
    assert cover(*HEADLINE, 25) == 2 and cover(*HEADLINE, 12) == 1


def test_budget_zero_and_bad_arguments(cover):
    assert cover(*HEADLINE, 0) == 0
    assert cover(*HEADLINE, 11) == 0 and cover(*HEADLINE, -5) == 0
    for bad in ((0, 10, 4), (10, 0, 4), (10, 10, 0), (-3, 10, 4)):
        assert cover(*bad, DEFAULT_MB * MB) == 0


def test_beyond_two_to_the_32(cover):
    w, h, n = 65536, 65536, 4                                       # w * h * samples = 2^34
    assert cover(w, h, n, 1 << 40) == 2 ** 34
    assert cover(w, h, n, 1 << 34) == (1 << 34) // 12
    big = 2 ** 31 - 1                                               # the product passes 2^63: the cover is the budget's
    assert span(big, big, big) > 2 ** 63
    assert cover(big, big, big, 2 ** 62) == 2 ** 62 // 12
    assert cover(big, big, big, 2 ** 63 - 1) == (2 ** 63 - 1) // 12


def test_never_more_than_the_budget_holds(cover):
    import random
    rng = random.Random(20261016)
    for _ in range(2000):
        w, h, n = (rng.choice((1, 2, 7, 64, 1080, 1920, 40000, 2 ** 31 - 1)) for _ in range(3))
        budget = rng.choice((0, 1, 12, 13, 4096, 100 * MB, DEFAULT_MB * MB, 2 ** 45, 2 ** 63 - 1))
        c = cover(w, h, n, budget)
        assert 0 <= c <= budget // 12
        assert c == min(span(w, h, n), budget // 12)
