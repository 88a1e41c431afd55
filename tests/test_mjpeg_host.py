"""Motion-JPEG, host side (no GPU): the decode oracle against Pillow, the JPEG header rules and their refusals, the AVI /
raw-stream containers behind ``open_video``, and ``csrc/jpeg_entropy.h`` -- the code the kernels run -- compiled into a
host program under AddressSanitizer and UBSan, on well-formed, truncated and garbage entropy data."""
import io
import shutil
import struct
import subprocess
import sys
import types

import numpy as np
import pytest

import jpeg_decode_oracle as jd
import mjpeg_cases as mc
from conftest import ROOT
from eioku_amd import frames as F
from eioku_amd import mjpeg as M


# ---- the oracle ----------------------------------------------------------------------------------------------------
def test_case_list_is_complete():
    assert len(mc.ENCODED) == 256 + 8 and len(set(mc.NAMES)) == len(mc.NAMES) == 256 + 8 + 32
    assert set(mc.files()) == set(mc.NAMES)


def test_oracle_equals_pillow_on_every_case():
    Image = pytest.importorskip("PIL.Image")
    for name, data in mc.files().items():
        ref = np.asarray(Image.open(io.BytesIO(data)))
        o = mc.oracle(name)
        assert o["status"] == 0, name
        assert np.array_equal(o["rgb"] if ref.ndim == 3 else o["luma"], ref), name


def test_oracle_equals_committed_pillow_pixels():
    px = mc.pillow_pixels()
    assert len(px) == 2 * 4 * 4 + 4  # two sizes, every sampling, every variant (q75rows exists at 33x47 only)
    for name, ref in px.items():
        o = mc.oracle(name)
        assert np.array_equal(o["rgb"] if ref.ndim == 3 else o["luma"], ref), name


def test_dht_stripped_files_decode_to_the_same_pixels():
    for c in mc.STRIPPED:
        a, b = mc.oracle(mc.name_of(*c)), mc.oracle(mc.name_of(*c, stripped=True))
        assert b"\xff\xc4" not in mc.files()[mc.name_of(*c, stripped=True)][:600] and np.array_equal(a["rgb"], b["rgb"])


def test_fixed_point_iteration_is_bounded_and_runs():
    data = mc.files()["40x56-noise-444-q75"]
    nbits = 8 * len(jd.parse(data)["segments"][0])
    r32, r1024 = jd.sync_rounds([data], 32), jd.sync_rounds([data], 1024)
    assert 2 <= r32 <= -(-nbits // 32) + 1 and 1 <= r1024 <= -(-nbits // 1024) + 1


# ---- JPEG headers ----------------------------------------------------------------------------------------------------
def test_parse_jpeg_agrees_with_the_oracle_on_every_case():
    for name, data in mc.files().items():
        p, f = jd.parse(data), M.parse_jpeg(data)
        assert f.geometry == (p["h"], p["w"], p["ncomp"], p["hs"] if p["ncomp"] == 3 else 1, p["vs"] if p["ncomp"] == 3 else 1), name
        assert f.pieces == p["segments"], name
        for c in range(p["ncomp"]):
            tq, td, ta = (int(v) for v in f.comp[c])
            assert np.array_equal(f.qtab[tq], p["qt"][p["comps"][c][0]]), name
            for cls, tid in ((0, td), (1, ta)):
                counts, symbols = p["dht"][(cls, p["comps"][c][1 + cls])]
                row = f.huff[cls * 2 + tid]
                assert list(row[:16]) == counts and list(row[16:16 + len(symbols)]) == symbols, name


def _patch(data: bytes, marker: int, offset: int, value: bytes) -> bytes:
    """``value`` written ``offset`` bytes into the body of the first ``marker`` segment."""
    at = data.index(bytes([0xFF, marker])) + 4 + offset
    return data[:at] + value + data[at + len(value):]


def _insert(data: bytes, marker: int, body: bytes) -> bytes:
    return data[:2] + bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body + data[2:]


def test_every_refusal_names_its_rule():
    ok = mc.files()["33x47-noise-420-q75"]
    sof = ok.index(b"\xff\xc0")
    cases = [
        (ok[:sof] + b"\xff\xc2" + ok[sof + 2:], "SOF2 .progressive.: only baseline SOF0"),
        (ok[:sof] + b"\xff\xc1" + ok[sof + 2:], "SOF1 .extended sequential.: only baseline SOF0"),
        (ok[:sof] + b"\xff\xc9" + ok[sof + 2:], "arithmetic coding is not supported"),
        (_insert(ok, 0xCC, b"\x00\x10"), "DAC marker: arithmetic coding"),
        (_patch(ok, 0xDB, 0, b"\x10"), "16-bit DQT"),
        (_patch(ok, 0xC0, 0, b"\x0c"), "12-bit samples"),
        (_patch(ok, 0xC0, 3, (9000).to_bytes(2, "big")), r"9000 x 47: width and height must be in \[1, 8192\]"),
        (_patch(ok, 0xC0, 7, b"\x12"), "sampling 1x2/1x1/1x1"),
        (_patch(ok, 0xC0, 7, b"\x41"), "sampling 4x1/1x1/1x1"),
        (_patch(ok, 0xC0, 10, b"\x21"), "sampling 2x2/2x1/1x1"),
        (_patch(ok, 0xDA, 0, b"\x01"), "a scan of 1 of 3 components: multiple scans"),
        (_patch(ok, 0xDA, 7, b"\x00\x05\x00"), "spectral selection"),
        (_insert(ok, 0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x00"), "Adobe APP14 transform 0"),
        (_insert(ok, 0xE0, b"AVI1\x01\x00\x00\x00"), "AVI1 field polarity 1: interlaced"),
        (ok[:-2] + b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00\x00\xff\xd9", "marker 0xda after the scan: multiple scans"),
        (b"RIFF" + ok, "no SOI"),
    ]
    for data, message in cases:
        with pytest.raises(M.UnsupportedJpeg, match=message):
            M.parse_jpeg(data)
    M.parse_jpeg(_insert(ok, 0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x01"))  # transform 1 is YCbCr
    M.parse_jpeg(_insert(ok, 0xE0, b"AVI1\x00\x00\x00\x00"))              # polarity 0: progressive frames
    four = ok[:sof] + b"\xff\xc0\x00\x14" + ok[sof + 4:sof + 9] + b"\x04" + ok[sof + 10:sof + 19] + b"\x04\x11\x00" + ok[sof + 19:]
    with pytest.raises(M.UnsupportedJpeg, match="4 components"):
        M.parse_jpeg(four)


def test_restart_segments_must_match_the_interval():
    data = mc.files()["33x47-noise-420-q75rows"]
    f = M.parse_jpeg(data)
    assert len(f.pieces) == 3 and f.mcus_per_piece == 3
    entropy, seg, qtab, huff, comp = M.pack([f, f])
    assert seg.shape == (6, 5) and seg[:, 0].tolist() == [0, 0, 0, 1, 1, 1] and seg[:, 1].tolist() == [0, 3, 6] * 2
    assert all(int(o) % 4 == 0 for o in seg[:, 3]) and entropy.size % 4 == 0
    for (_, _, _, off, nbits), piece in zip(seg.tolist(), f.pieces * 2):
        assert entropy[off:off + nbits // 8].tobytes() == piece
    cut = data.index(b"\xff\xd1")
    with pytest.raises(M.UnsupportedJpeg, match="2 restart segments for 3 restart intervals"):
        M.parse_jpeg(data[:cut] + data[cut + 2:])


# ---- containers ------------------------------------------------------------------------------------------------------
class CountingFile(io.BytesIO):
    """Records every read as (offset, bytes returned)."""

    def __init__(self, data):
        super().__init__(data)
        self.reads = []

    def read(self, n=-1):
        at = self.tell()
        out = super().read(n)
        self.reads.append((at, len(out)))
        return out


def _frames(n=6):
    names = ["16x16-noise-420-q75", "16x16-noise-420-q100", "16x16-noise-420-q20opt", "16x16-smooth-420-q75",
             "16x16-smooth-420-q100", "16x16-noise-420-q75-nodht"]
    return [mc.files()[names[i % len(names)]] for i in range(n)]


def test_avi_writer_pins_the_header_struct_sizes():
    """Literal offsets, so that the writer and the parser cannot share a mistake about the three header structs."""
    avi = mc.avi_bytes(_frames(3), 30000, 1001, 16, 16)
    at = avi.index(b"avih")
    assert avi[at + 4:at + 8] == (56).to_bytes(4, "little") and avi[at + 8 + 56:at + 8 + 60] == b"LIST"
    at = avi.index(b"strh")
    assert avi[at + 4:at + 8] == (56).to_bytes(4, "little") and avi[at + 8:at + 16] == b"vidsMJPG"
    assert struct.unpack("<II", avi[at + 8 + 20:at + 8 + 28]) == (1001, 30000) and avi[at + 8 + 56:at + 8 + 60] == b"strf"
    at = avi.index(b"strf")
    assert avi[at + 4:at + 8] == (40).to_bytes(4, "little") and avi[at + 8 + 16:at + 8 + 20] == b"MJPG"
    assert struct.unpack("<ii", avi[at + 8 + 4:at + 8 + 12]) == (16, 16) and avi[at + 8 + 40:at + 8 + 44] == b"LIST"


def test_avi_parsing_of_an_awkward_file():
    jpegs = _frames(6)
    assert any(len(j) & 1 for j in jpegs), "an odd-sized video chunk is part of the test"
    frames = jpegs[:3] + [None] + jpegs[3:]  # a zero-length chunk: frame 3 repeats frame 2
    avi = mc.avi_bytes(frames, 30000, 1001, 16, 16, awkward=True)
    assert b"idx1" not in avi and b"JUNK" in avi and b"01wb" in avi and b"rec " in avi and b"AVIX" in avi
    src = M.MjpegSource("clip.avi", file=CountingFile(avi))
    assert src.total_frames == 7 and src.time_base == (1001, 30000)
    assert src.fps == pytest.approx(30000 / 1001) and src.duration_s == pytest.approx(7 * 1001 / 30000)
    expect = jpegs[:3] + [jpegs[2]] + jpegs[3:]
    assert [src.frame_bytes(i) for i in range(7)] == expect
    for name, fourcc in (("lower case", b"mjpg"), ("JPEG", b"JPEG")):
        assert M.MjpegSource("clip.avi", file=io.BytesIO(mc.avi_bytes(jpegs, fourcc=fourcc))).total_frames == 6, name
    with pytest.raises(M.NotMjpeg, match="'H264' is not Motion-JPEG"):
        M.MjpegSource("clip.avi", file=io.BytesIO(mc.avi_bytes(jpegs, fourcc=b"H264")))
    with pytest.raises(RuntimeError, match="begins with a zero-length"):
        M.MjpegSource("clip.avi", file=io.BytesIO(mc.avi_bytes([None] + jpegs)))


def test_grab_never_reads_the_payload():
    jpegs = _frames(6)
    avi = mc.avi_bytes(jpegs, awkward=True)
    f = CountingFile(avi)
    src = M.MjpegSource("clip.avi", file=f)
    spans = [(avi.index(j), len(j)) for j in jpegs[:5]]  # the sixth file's bytes equal no other chunk's either
    assert all(n <= 56 for _, n in f.reads), "opening reads chunk headers and the three header structs only"
    f.reads.clear()
    for _ in range(4):
        assert src.grab()
    assert f.reads == []
    ok, data = src.read_encoded()
    assert ok and data == jpegs[4] and f.reads == [spans[4]]
    assert src.grab() and not src.grab() and src.read_encoded() == (False, None)


def test_open_video_returns_the_mjpeg_source(tmp_path):
    jpegs = _frames(5)
    (tmp_path / "a.avi").write_bytes(mc.avi_bytes(jpegs, 25, 1, 16, 16))
    (tmp_path / "b.mjpeg").write_bytes(b"".join(jpegs))
    (tmp_path / "c.MJPG").write_bytes(b"".join(jpegs[:2]))
    (tmp_path / "c.MJPG.json").write_text('{"fps": 29.97, "time_base": [1001, 30000]}')
    (tmp_path / "d.jpg").write_bytes(jpegs[0])
    (tmp_path / "e.jpeg").write_bytes(jpegs[0])
    for name, n, fps in (("a.avi", 5, 25.0), ("b.mjpeg", 5, 25.0), ("c.MJPG", 2, 29.97), ("d.jpg", 1, 25.0), ("e.jpeg", 1, 25.0)):
        src = F.open_video(str(tmp_path / name))
        assert isinstance(src, M.MjpegSource) and src.total_frames == n and src.fps == fps, name
        assert src.frame_bytes(n - 1) == jpegs[n - 1]
        src.release()
    assert F.open_video(str(tmp_path / "c.MJPG")).time_base == (1001, 30000)


def test_an_avi_with_another_codec_still_goes_to_cv2(tmp_path, monkeypatch):
    (tmp_path / "h.avi").write_bytes(mc.avi_bytes(_frames(2), fourcc=b"H264"))
    cv2 = types.ModuleType("cv2")
    cv2.CAP_PROP_FPS, cv2.CAP_PROP_FRAME_COUNT = 5, 7
    cv2.VideoCapture = lambda path: types.SimpleNamespace(get=lambda prop: 2.0)
    monkeypatch.setitem(sys.modules, "cv2", cv2)
    assert isinstance(F.open_video(str(tmp_path / "h.avi")), F.Cv2FrameSource)
    assert isinstance(F.open_video("/no/such/file.avi"), F.Cv2FrameSource)


# ---- the entropy code of the kernels, on the host, under sanitizers ------------------------------------------------------
HOST_FIXTURES = ["33x47-noise-420-q75", "40x56-noise-422-q20opt", "94x95-noise-444-q90rst", "17x9-smooth-grey-q100"]


def test_entropy_header_in_a_sanitized_host_program(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    blob = [struct.pack("<i", len(HOST_FIXTURES))]
    for name in HOST_FIXTURES:
        f = M.parse_jpeg(mc.files()[name])
        entropy, seg, qtab, huff, comp = M.pack([f])
        coef = mc.oracle(name)["coef"]
        blob += [struct.pack("<8i", f.h, f.w, f.ncomp, f.hs, f.vs, len(seg), entropy.size, coef.shape[0]), seg.tobytes(), huff.tobytes(),
                 comp.tobytes() + bytes(3), entropy.tobytes(), coef.tobytes()]
    (tmp_path / "fixtures.bin").write_bytes(b"".join(blob))
    exe = tmp_path / "mjpeg_entropy_host"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", str(ROOT / "eioku_amd" / "csrc"), str(ROOT / "tests" / "mjpeg_entropy_host.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe), str(tmp_path / "fixtures.bin")], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    for k, name in enumerate(HOST_FIXTURES):  # the host program's round count is the oracle's
        assert f"fixture {k} rounds32 {jd.sync_rounds([mc.files()[name]], 32)}\n" in run.stdout, name
