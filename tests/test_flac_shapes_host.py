"""The FLAC streams of tests/flac_write_util.py on the CPU: the oracle decodes each one to the PCM the writer encoded (the writer and the oracle
share no code, so this is the independent check of both), and each case really holds the bitstream shape it is there for — read back out of the
written bytes.  tests/test_gpu_flac_shapes.py then holds the kernels to the oracle on the same streams."""
import numpy as np
import pytest

from tests import flac_write_util as W

BATCHES = sorted(W.batches())


def _flat(batch):
    return [h for s in batch.values() for fr in s.subframe_headers() for h in fr]


@pytest.mark.parametrize("name", BATCHES)
def test_oracle_restores_the_encoded_pcm(oracle, name):
    for sn, s in W.batches()[name].items():
        ref = oracle.flac(s.data)
        assert ref.channels == s.channels and ref.sample_rate == s.rate, sn
        for c, want in enumerate(s.expected()):
            assert np.array_equal(ref.data[c], want), (sn, c)
            inside = np.abs(s.pcm[:, c]) < 2 ** (s.depth - 1)    # beyond the depth's range the reference wraps once (:504)
            assert np.array_equal((ref.data[c] * 2.0 ** s.depth)[inside], s.pcm[inside, c].astype(np.float64)), (sn, c)


def test_writer_agrees_with_gen_flac(oracle):
    """an ordinary 16-bit stereo signal: what the writer makes of it and what oracle.gen_flac makes of it decode to the same samples"""
    pcm = W.ordinary_pcm(5 * 1024 + 300, 2, 7)
    mine = W.encode_stream(pcm, 16, 1024, W._e_plan, asgn=W._e_asgn)
    a, b = oracle.flac(mine.data), oracle.flac(oracle.gen_flac(pcm.ravel(), 2, 16, 44100, 1024))
    for c in range(2):
        assert np.array_equal(a.data[c], b.data[c]) and np.array_equal(a.data[c] * 65536.0, pcm[:, c].astype(np.float64))


# ---------------------------------------------------------------- the shapes, read back from the bytes
@pytest.mark.parametrize("name", [n for n in BATCHES if n.startswith("A-method1-") and n[10].isdigit()])
def test_A_holds_method_1_parameters_and_escapes(name):
    batch = W.batches()[name]
    lead = set()
    for h in _flat(batch):
        lead.add((h["method"], h["param0"], h.get("escape_bits0")))
        assert h["porder"] == 2
    assert {(1, k, None) for k in (0, 14, 15, 16, 23, 30)} | {(1, 31, w) for w in (0, 1, 25, 31)} | {(0, 14, None)} <= lead
    assert all(fh["blocksize"] == 256 for s in batch.values() for fh in s.frame_headers())
    if "2ch" in name:
        assert any({h["method"] for h in fr} == {0, 1} for s in batch.values() for fr in s.subframe_headers())    # both methods in one frame


def test_A_beyond_int32_holds_a_quotient_past_int32():
    s = W.batches()["A-method1-beyond-int32"]["0"]
    h = s.subframe_headers()[0][0]
    assert (h["method"], h["param0"], h["kind"], h["order"]) == (1, 30, "fixed", 0)
    assert np.max(np.abs(s.pcm)) > 2 ** 32


@pytest.mark.parametrize("depth", [16, 24])
def test_B_holds_long_predictors(depth):
    batch = W.batches()[f"B-long-predictors-{depth}bit"]
    seen = set()
    for s in batch.values():
        fhs, subs = s.frame_headers(), s.subframe_headers()
        bs = fhs[0]["blocksize"]
        assert bs in (64, 4096) and (bs != 64 or len(fhs) >= 70)
        for (h,) in subs:
            assert h["kind"] == "lpc" and (bs >> h["porder"]) >= h["order"]      # prediction itself, not the warm-up overwrite of :400
            seen.add((bs, h["order"], h["precision"], sum(abs(c) for c in h["coefs"]) < 2 ** 15, h["porder"] if bs == 64 else None))
    for bs in (64, 4096):
        for order in (13, 16, 31, 32):
            for prec in (15, 16):
                for small in (False, True):
                    for po in ((0, 1) if bs == 64 else (None,)):
                        assert (bs, order, prec, small, po) in seen


@pytest.mark.parametrize("depth", [16, 24])
def test_C_holds_the_shifts(depth):
    hs = _flat(W.batches()[f"C-shifts-{depth}bit"])
    assert {(h["shift"], h["order"]) for h in hs} == {(s, o) for s in (-16, -4, -1, 0, 15) for o in (1, 2, 8)}
    assert all(h["kind"] == "lpc" for h in hs)
    wide = W.batches()["C-shift-beyond-int32"]["0"]
    assert wide.subframe_headers()[0][0]["shift"] == -1 and np.max(wide.pcm) > 2 ** 32


@pytest.mark.parametrize("ch", [3, 6, 8])
def test_D_holds_the_channels(ch):
    batch = W.batches()[f"D-{ch}-channels"]
    assert {fh["bs_code"] for s in batch.values() for fh in s.frame_headers()} == {1, 7}
    assert {fh["blocksize"] for s in batch.values() for fh in s.frame_headers()} == {192, 1000}
    for s in batch.values():
        for fh, fr in zip(s.frame_headers(), s.subframe_headers()):
            assert fh["chan_asgn"] == ch - 1 and len(fr) == ch
            assert [h["wasted"] for h in fr] == [0, 2] + [0] * (ch - 2)
        assert {h["kind"] for fr in s.subframe_headers() for h in fr} == {"constant", "verbatim", "fixed", "lpc"}


def test_E_holds_the_metadata_blocks():
    b = W.batches()["E-metadata"]
    types = lambda n: [t for t, _, _ in W.read_metadata(b[n].data)[0]]
    lens = lambda n: [l for _, l, _ in W.read_metadata(b[n].data)[0]]
    assert types("padding") == [1, 0, 1] and lens("padding") == [0, 34, 8191]
    assert types("application-seektable") == [2, 0, 3]
    assert types("comment-picture-unknown") == [4, 0, 6, 126]
    assert types("two-streaminfos") == [0, 1, 0]
    s = b["two-streaminfos"]
    first, second = [s.data[o:o + 34] for t, _, o in W.read_metadata(s.data)[0] if t == 0]
    assert first[10:18] != second[10:18]
    # the stuffed PICTURE: sync codes with a good CRC-8 in front of the first frame
    s = b["comment-picture-unknown"]
    pic = next(o for t, _, o in W.read_metadata(s.data)[0] if t == 6)
    at = s.data.index(b"\xff\xf8", pic)
    h = W.read_frame_header(s.data, at)
    assert at < s.frame_at[0] and h["crc_ok"] and h["chan_asgn"] == 1 and h["ss_code"] == 4
    # the type-4 quirk: the declared length and the content disagree, and the first frame sits behind the CONTENT
    for n, sign in (("comment-declared-long", 1), ("comment-declared-short", -1)):
        s = b[n]
        (_, _, _), (t, declared, o) = W.read_metadata(s.data)[0]
        assert t == 4 and s.data[o:o + len(W.VC)] == W.VC and (declared - len(W.VC)) * sign > 0
        first = o + len(W.VC)
        assert W.read_frame_header(s.data, first)["sync"] == 0x3FFE and W.read_frame_header(s.data, first)["crc_ok"]
        assert s.data[o + declared:o + declared + 2] != b"\xff\xf8" or sign > 0


def test_E_error_files(oracle):
    for name, (data, what) in W.error_files().items():
        if what == "empty":
            a = oracle.flac(data)
            assert a.channels == 2 and all(len(d) == 0 for d in a.data), name
        else:
            with pytest.raises(oracle.OracleError) as e:
                oracle.flac(data)
            assert what in str(e.value), name


def test_F_holds_the_header_fields():
    b = W.batches()["F-header-fields"]
    H = {n: s.frame_headers() for n, s in b.items()}
    assert all(8 <= len(h) <= 40 or n == "blocksize-65536-code-7" for n, h in H.items())
    every = lambda n, **kw: all(all(h[k] == v for k, v in kw.items()) for h in H[n])
    assert every("rate-code-12", rate_code=12, crc_ok=True) and every("rate-code-13", rate_code=13, crc_ok=True)
    assert every("sample-size-contradicts", ss_code=6, crc_ok=True)
    assert every("reserved-bit-1", reserved=1) and every("reserved-bit-2", reserved2=1)
    assert every("strategy-7-byte-number", strategy=1, number_bytes=7, crc_ok=True) and every("strategy-8-byte-number", strategy=1, number_bytes=8, crc_ok=True)
    assert every("bad-crc8-every-frame", crc_ok=False) and len(H["bad-crc8-every-frame"]) == 40
    assert every("blocksize-1-code-6", bs_code=6, blocksize=1) and every("blocksize-256-code-6", bs_code=6, blocksize=256)
    assert every("blocksize-257-code-7", bs_code=7, blocksize=257)
    assert every("blocksize-65536-code-7", bs_code=7, blocksize=65536) and len(H["blocksize-65536-code-7"]) == 1
    h = b["blocksize-65536-code-7"].subframe_headers()[0][0]
    assert (h["kind"], h["order"]) == ("fixed", 2)
    # the next frame starts where this one's header says: every frame header parses at its recorded offset
    assert all(h["sync"] == 0x3FFE for hs in H.values() for h in hs)


# ---------------------------------------------------------------- 32-bit: BitInputStream.readUint / readSignedInt restated (:351-369)
class LuaBits:
    def __init__(self, data, pos):
        self.data, self.pos, self.buf, self.len = data, pos, 0, 0
        self.phases = set()

    def uint(self, n):
        if n == 0:
            return 0
        if n >= 32:
            self.phases.add(self.len % 8)
        while self.len < n:
            self.buf = (self.buf * 256 + self.data[self.pos]) % 0x100000000000
            self.pos += 1
            self.len += 8
        self.len -= n
        r = self.buf >> self.len
        return r % (1 << n) if n < 32 else r

    def sint(self, n):
        v = self.uint(n)
        return v - (1 << n) if v >= 1 << (n - 1) else v


def lua_decode_verbatim(s):
    """decodeFrame / decodeSubframes (:472-567) for a stream whose subframes are all verbatim without wasted bits"""
    r = LuaBits(s.data, s.frame_at[0])
    out = [[] for _ in range(s.channels)]
    for _ in s.frame_at:
        assert r.uint(14) == 0x3FFE
        r.uint(2); bsc = r.uint(4); r.uint(4); asgn = r.uint(4); r.uint(4); r.uint(8)
        bs = r.uint(8) + 1 if bsc == 6 else W.BS_BY_CODE[bsc]
        r.uint(8)
        sub = []
        for c in range(s.channels):
            d = s.depth + (1 if (asgn, c) in ((8, 1), (9, 0), (10, 1)) else 0)
            assert r.uint(8) == 2    # verbatim, no wasted bits
            sub.append([r.sint(d) for _ in range(bs)])
        if asgn == 8:
            sub[1] = [a - b for a, b in zip(sub[0], sub[1])]
        elif asgn == 9:
            sub[0] = [a + b for a, b in zip(sub[0], sub[1])]
        elif asgn == 10:
            right = [a - (b >> 1) for a, b in zip(sub[0], sub[1])]
            sub[0], sub[1] = [a + b for a, b in zip(right, sub[1])], right
        for c in range(s.channels):
            out[c] += [(v - (1 << s.depth) if v >= 1 << (s.depth - 1) else v) / 2.0 ** s.depth for v in sub[c]]
        r.len -= r.len % 8
        r.uint(16)
    return [np.array(o) for o in out], r.phases


@pytest.mark.parametrize("name", ["G-32bit-mono", "G-32bit-stereo"])
def test_G_32bit_quirk_is_live_and_restated(oracle, name):
    batch = W.quirk_batches()[name]
    for sn, s in batch.items():
        assert s.depth == 32 and all(h["ss_code"] == 7 for h in s.frame_headers())
        ref = oracle.flac(s.data)
        assert any(not np.array_equal(ref.data[c], s.expected()[c]) for c in range(s.channels)), sn    # the stale high bits change samples
    s = batch["verbatim"]
    want, phases = lua_decode_verbatim(s)
    ref = oracle.flac(s.data)
    for c in range(s.channels):
        assert np.array_equal(ref.data[c], want[c]), c
    if s.channels == 2:
        assert {h["chan_asgn"] for h in s.frame_headers()} == {1, 8, 9, 10}
        assert phases == set(range(8))      # reads of 32 / 33 bits begin at every bitBufferLen % 8
        assert {h["chan_asgn"] for h in batch["fixed-2"].frame_headers()} == {1, 8, 9, 10}
    assert {h["kind"] for fr in batch["fixed-2"].subframe_headers() for h in fr} >= {"fixed"}


# ---------------------------------------------------------------- H's special streams
def test_H_streams(oracle):
    s = W.h_declining()
    ref = oracle.flac(s.data)
    assert np.array_equal(ref.data[0], s.expected()[0])
    mid = s.subframe_headers()[len(s.frame_at) // 2]
    assert mid[0]["order"] == 20 and s.frame_headers()[len(s.frame_at) // 2]["blocksize"] == 16
    s = W.h_beyond_int16()
    ref = oracle.flac(s.data)
    assert np.array_equal(ref.data[0], s.expected()[0]) and np.array_equal(ref.data[1], s.expected()[1])
    assert ref.data[1].min() == -98303 / 65536 and s.frame_headers()[3]["chan_asgn"] == 8
