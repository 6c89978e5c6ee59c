"""The table of tests/rate_edges_util.py, proven on the CPU: every row's guard share lies on its stated side, the 32-bit division the kernels
rely on is exact over everything an inside row can ask of it, the phase tables sum to one, and the reference alone stays within the
neighbouring-float cap that tests/test_gpu_rate_edges.py holds the level-1 kernels to."""
import numpy as np
import pytest

from tests import rate_edges_util as U


@pytest.mark.parametrize("row", U.ROWS, ids=lambda r: r.id)
def test_row_is_what_the_guard_computes(row):
    ok, a, b, t, s = U.fast_eligible(row.old, row.new)
    assert (a, b, t) == (row.a, row.b, row.T), (a, b, t)
    assert abs(s - row.s) <= 5e-3 * row.s, (s, row.s)                      # the table's figure, to the digits it gives
    assert ok == (row.side == U.INSIDE), (ok, row.side)
    assert (row.side == U.REFUSED) == U.lds_refused(a, b, t)
    if row.side == U.INSIDE:
        assert s < 1
    if row.side == U.OUTSIDE:
        assert s >= 1
    if row.band:
        assert (0.9 <= s < 1) if row.side == U.INSIDE else (1 <= s <= 1.1), s
    # the T step-down: the chosen T is the largest of 4096 / 3072 / 2048 / 1024 whose window fits 40 KiB, or 1024
    for t2 in (4096, 3072, 2048):
        if t2 > t:
            assert (t2 * a / b + 64) * 4 > 40 * 1024
    assert t == 1024 or (t * a / b + 64) * 4 <= 40 * 1024


def test_the_guard_in_doubles_agrees_with_the_integers():
    """fast.hip:218-220 evaluates the rules in doubles; the helper in integers.  Every product here is far below 2^53, so the two agree — shown on the
    rows, and on the rates either side of each LDS threshold"""
    for old, new in [(r.old, r.new) for r in U.ROWS] + [(o, 48000) for o in (119250, 119251, 159000, 159001, 238500, 238501, 717000, 717001)]:
        a, b = U.reduce_rates(old, new)
        t = 4096
        while t > 1024 and (float(t) * float(a) / float(b) + 64) * 4 > 40 * 1024:
            t -= 1024
        assert t == U.tile_out(a, b), (old, new)
        assert ((float(t) * float(a) / float(b) + 64) * 4 > 60 * 1024) == U.lds_refused(a, b, t), (old, new)
        assert ((float(b) + float(t) * float(a)) * float(b) >= 4294967296.0) == ((b + t * a) * b >= U.TWO32), (old, new)


def test_reduction_and_doubling():
    assert U.reduce_rates(44100, 48000) == (147, 160)
    assert U.reduce_rates(48000, 48000) == (2, 2) and U.reduce_rates(96000, 48000) == (4, 2) and U.reduce_rates(720000, 48000) == (30, 2)   # b < 2: 2a / 2
    assert U.reduce_rates(24000, 48000) == (1, 2) and U.reduce_rates(1, 48000) == (1, 48000)
    assert U.reduce_rates(47999, 48000) == (47999, 48000) and not U.fast_eligible(47999, 48000)[0]        # the suite's old "odd rate": s = 2.2e6
    for old in (47999, 8001, 44056):
        assert U.fast_eligible(old, 48000)[4] > 30                                                       # far outside (8001 Hz: 2667 / 16000, s = 31.5): they only ever met the fallback


def test_no_eligible_rate_toward_48k_lies_nearer_the_guard_than_the_table():
    """the table holds the extremes of a full enumeration: nothing eligible lies above s(3132 Hz), nothing refused below s(4905 Hz), and the largest b
    that exists (48000: the 1 Hz row's, shared by every rate coprime to 48000 up to 7 Hz) stays eligible"""
    best_in, best_out, big_b = (0, 0), (9e9, 0), (0, 0)
    for old in range(1, 48001):
        ok, a, b, t, s = U.fast_eligible(old, 48000)
        if ok:
            best_in = max(best_in, (s, old))
            big_b = max(big_b, (b, old))
        else:
            best_out = min(best_out, (s, old))
    assert best_in[1] == 3132 and best_out[1] == 4905 and big_b == (48000, 7), (best_in, best_out, big_b)
    assert "3132-48000" in U.BY_ID and "4905-48000" in U.BY_ID and U.BY_ID["1-48000"].b == 48000


@pytest.mark.parametrize("row", [r for r in U.ROWS if r.side == U.INSIDE], ids=lambda r: r.id)
def test_division_is_exact_for_every_n_an_inside_row_can_meet(row):
    """q = (n * ceil(2^32 / b)) >> 32 equals n // b for ALL n < b + T a: a tile's first position is below b, its last adds (T - 1) a"""
    assert U.division_holds(row.b, row.b + row.T * row.a) is None
    # the (dq64, dr64) walk: 64 outputs further is dq64 source samples and dr64 of b phases, with one carry at most
    dq, dr = 64 * row.a // row.b, 64 * row.a % row.b
    rem = np.arange(row.b, dtype=np.int64)
    carry = (rem + dr) >= row.b
    assert np.array_equal((rem + 64 * row.a) // row.b, dq + carry) and np.array_equal((rem + 64 * row.a) % row.b, rem + dr - carry * row.b)


@pytest.mark.parametrize("row", [r for r in U.ROWS if r.side == U.OUTSIDE], ids=lambda r: r.id)
def test_guard_is_not_idle_outside(row):
    """outside rows: the guard's bound is sufficient, not tight — but the multiply-high does go wrong not far beyond it, so the refusal protects
    something: some n < 2^32 has the wrong quotient"""
    m, b = U.magic(row.b), row.b
    e = m * b - U.TWO32                              # q is exact while n e < 2^32 (roughly): the first failure is near 2^32 / e
    assert 0 < e < b
    n0 = (U.TWO32 // e // b) * b + b - 1             # a residue b - 1 just past that point
    bad = [n for n in range(n0, min(n0 + 4 * b, U.TWO32), b) if (n * m) >> 32 != n // b]
    assert bad, (row.id, e, n0)


@pytest.mark.parametrize("row", [r for r in U.ROWS if r.side == U.INSIDE], ids=lambda r: r.id)
def test_tile_guards_cannot_refuse_an_eligible_row(row):
    for site, tile in U.TILE_GUARDS.items():
        if site.startswith("rs_periodic") and not (row.a < row.b and 320 * row.a % row.b == 0):
            continue                                  # rsp_try declines first (rs_periodic.hip:432)
        assert tile <= row.T and (row.b + tile * row.a) * row.b < U.TWO32, site
    if row.a < row.b and 320 * row.a % row.b == 0:
        assert row.b <= 320 and U.share(row.a, row.b, 1280) < 0.031


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("row", [r for r in U.ROWS if r.side == U.INSIDE and r.b <= 512], ids=lambda r: r.id)
def test_phase_weights_sum_to_one(row, interp):
    w = U.phase_weights(row.b, interp)
    r = np.arange(row.b)
    if interp == "linear":
        assert np.array_equal(w, r / row.b)          # fx = r / b, correctly rounded
        assert w[0] == 0 and np.all(np.diff(w) > 0) and w[-1] < 1
    else:
        assert w.shape == (row.b, 4)
        assert np.max(np.abs(w.sum(1) - 1)) <= 2.3e-16          # four roundings to fp64: an ulp of 1
        assert tuple(w[0]) == (0.0, 1.0, 0.0, 0.0)             # phase 0 copies the tap
        f = r / row.b
        assert np.max(np.abs(w @ np.array([-1.0, 0.0, 1.0, 2.0]) - f)) <= 4e-16   # the cubic reproduces a straight line: the weights' first moment is fx


@pytest.mark.parametrize("br", U.BLOCK_ROWS, ids=lambda r: r.id)
def test_block_rows(br):
    assert U.reduce_rates(br.rate, 48000) == (br.fa, br.fb)
    nout = {"ima": U.ima_newlen_full, "msadpcm": U.ms_newlen}[br.family](br.rate, br.block) if br.family != "tail" else U.out_count(br.block, br.rate, 48000)
    s = U.block_share(nout, br.fa, br.fb)
    assert nout == br.nout and abs(s - br.s) <= 5e-3 * br.s, (nout, s)
    assert (s < 1) == (br.side == U.INSIDE)
    if not br.what:
        assert (0.9 <= s < 1) if br.side == U.INSIDE else (1 <= s <= 1.1), s
    if br.side == U.INSIDE:
        assert U.division_holds(br.fb, nout * br.fa + br.fb) is None
    if br.family != "ima":
        assert br.fb <= 512                                                      # the other half of msadpcm.hip:1062 / stream_tail.hip:355
    if br.family == "ima":
        assert br.block > 4 and (br.block - 4) % 4 == 0                          # codecs.hip:1408


def test_ima_f32_kernel_never_reaches_the_guard():
    """k_ima_stream_f32 needs fb <= 512 (codecs.hip:1531) and its LDS (:1551-1553) caps block_align near 2 KiB: with those, s stays below 0.25 — the
    per-block guard only ever switches P.fast inside k_ima_stream (fb > 512), which is why both IMA rows name that kernel"""
    worst = 0.0
    for fb in (480, 500):
        ba = 4
        while True:
            ba += 4
            capf = (((ba - 4) * 2 + 8 + 8 + 15) & ~15)                           # + IMA_DL_CAP >= 0: a lower bound of the LDS
            if (((fb * 4 + 3) & ~3) + 96) * 4 + capf * 4 * 4 > 64 * 1024:
                break
            worst = max(worst, U.block_share(int((ba - 4) * 2 * fb / (fb - 1)), fb - 1, fb))
    assert worst < 0.25, worst


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("row", [r for r in U.ROWS if U.level1_on_exact_positions(r)], ids=lambda r: r.id)
def test_reference_alone_stays_within_the_neighbouring_float_cap(oracle, row, interp):
    """The level-1 bound of tests/test_gpu_rate_edges.py: every stored f32 within one f32 spacing of the oracle's double rounded to f32, at most
    max(2, total // 500) of them on the neighbouring float.  The kernels' position is the exact rational, the oracle's the rounded double
    (i - 1) / ratio + 1: an fp64 numpy evaluation at the exact positions, rounded once, must itself meet that bound on the streams the GPU test
    uses — then a failure on the GPU can only be the kernel's.  (Rows that level 1 hands to the reference-order kernel, U.DECLINES, take the oracle's
    own position: nothing to show there.)"""
    diff = total = 0
    worst = 0.0
    for s in U.s16_streams(row):
        ref = oracle.resample(oracle.pcm(s.tobytes(), 16, oracle.SIGNED, 1, row.old), row.new, oracle.INTERP[interp]).data[0]
        assert len(ref) == U.out_count(len(s), row.old, row.new)
        dec = np.where(s < 0, s / 32768.0, s / 32767.0)
        got = U.exact_position_resample(dec, row.a, row.b, len(ref), interp)
        r32 = ref.astype(np.float32)
        worst = max(worst, float(np.max(np.abs(got.astype(np.float32).astype(np.float64) - r32.astype(np.float64)), initial=0)))
        diff += int(np.count_nonzero(got.astype(np.float32) != r32))
        total += len(ref)
    print(f"{row.id} {interp}: exact-position fp64 vs oracle: {diff} of {total} outputs on the neighbouring float (cap {max(2, total // 500)}), worst {worst:.3e}")
    assert worst <= 1.2e-7
    assert diff <= max(2, total // 500), (diff, total)


@pytest.mark.parametrize("fmt,interp", [("s24", "linear"), ("s24", "cubic"), ("g711", "linear"), ("g711", "cubic")])
@pytest.mark.parametrize("row", [r for r in U.ROWS if U.level1_on_exact_positions(r)], ids=lambda r: r.id)
def test_dyadic_formats_reference_share_is_rounding_boundaries_only(oracle, row, fmt, interp):
    """24-bit PCM (v / 2^23 for v < 0) and G.711 (m / 2^13) decode to dyadic fractions.  At a dyadic phase — b = 160, 320, 384 have them — the
    interpolated double is a short dyadic number that lies EXACTLY between two floats about once in sixteen, and the oracle's rounded position
    decides such a tie by its own last bits: there the reference alone exceeds max(2, total // 500) (1.3 % of the outputs at 44100 Hz, 24-bit,
    linear).  tests/test_gpu_rate_edges.py therefore grants the kernel that cap ON TOP of this count (`ref_diff`), which is sound only if the
    count holds nothing but rounding boundaries: every output at which the exact-position fp64 value and the oracle round apart lies within
    2^-35 of the midpoint of two floats, and within one f32 spacing."""
    from tests.util import pcm16, signal
    diff = total = off_boundary = 0
    for i, n in enumerate(U.source_lengths(row)):
        a = (oracle.pcm(U.s24_bytes(signal(n, row.old, 4, 2 * i)), 24, oracle.SIGNED, 1, row.old) if fmt == "s24" else
             oracle.g711(oracle.gen_g711(pcm16(n, row.old, 5, i), True), True, 1, row.old))
        ref = oracle.resample(a, row.new, oracle.INTERP[interp]).data[0]
        got = U.exact_position_resample(a.data[0], row.a, row.b, len(ref), interp)
        g32, r32 = got.astype(np.float32), ref.astype(np.float32)
        mm = g32 != r32
        assert np.max(np.abs(g32.astype(np.float64) - r32.astype(np.float64)), initial=0) <= 1.2e-7
        mid = (g32.astype(np.float64) + r32.astype(np.float64)) / 2           # where the two round apart they are neighbours: the boundary between them
        off_boundary += int(np.count_nonzero(mm & (np.abs(ref - mid) > 2.0 ** -35)))
        diff += int(mm.sum())
        total += len(ref)
    print(f"{row.id} {fmt} {interp}: the reference alone: {diff} of {total} on the neighbouring float (cap {max(2, total // 500)})")
    assert off_boundary == 0, (off_boundary, diff, total)
