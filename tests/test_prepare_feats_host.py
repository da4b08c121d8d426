"""Host side of the feature-preparation stage (no GPU): misc/tools/filter_data_dir.py's two rules and the consistency of its four files,
the command line of nnet/lib/prepare_feats.py as _cli.py declares it, and the checks and offset arithmetic of ops.cm_encode."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")


def _cli():
    sys.path.insert(0, os.path.join(PKG, "nnet", "lib"))
    try:
        import _cli
        return _cli
    finally:
        sys.path.pop(0)


def _write_dir(root, frames, spk_of, feats=None):
    os.makedirs(root)
    order = list(frames)[::-1]      # unsorted on purpose
    open(os.path.join(root, "utt2num_frames"), "w").write("".join("%s %d\n" % (u, frames[u]) for u in order))
    open(os.path.join(root, "utt2spk"), "w").write("".join("%s %s\n" % (u, spk_of[u]) for u in sorted(spk_of)))
    feats = {u: "/data/feats.ark:%d" % (17 * i + 6) for i, u in enumerate(frames)} if feats is None else feats
    open(os.path.join(root, "feats.scp"), "w").write("".join("%s %s\n" % (u, rx) for u, rx in feats.items()))
    open(os.path.join(root, "spk2utt"), "w").write("stale line\n")
    open(os.path.join(root, "vad.scp"), "w").write("left alone\n")
    return feats


def _read(root, name):
    return [ln.split() for ln in open(os.path.join(root, name))]


def test_filter_data_dir_rules_and_consistency(tmp_path):
    from tf_kaldi_speaker_amd.misc.tools import filter_data_dir
    frames = {"B-u1": 401, "B-u2": 400, "B-u3": 900, "A-u1": 500, "A-u2": 450, "a-u1": 1000, "C-u1": 399, "C-u2": 2, "Z-u9": 700}
    spk_of = {u: u.split("-")[0] for u in frames}
    spk_of["Q-u1"] = "Q"                                   # in utt2spk only: no features, dropped
    root = str(tmp_path / "train")
    feats = _write_dir(root, frames, spk_of)
    # frames > 400 first: B-u2 (= 400), C-u1, C-u2 leave; then speakers with >= 2 REMAINING utterances: B (2 left) and A stay, a, Z leave
    assert filter_data_dir.filter_data_dir(root, min_len=400, min_num_utts=2) == (4, 2)
    utts = ["A-u1", "A-u2", "B-u1", "B-u3"]                # C order: upper case before lower case
    assert _read(root, "utt2num_frames") == [[u, str(frames[u])] for u in utts]
    assert _read(root, "utt2spk") == [[u, spk_of[u]] for u in utts]
    assert _read(root, "feats.scp") == [[u, feats[u]] for u in utts]
    assert _read(root, "spk2utt") == [["A", "A-u1", "A-u2"], ["B", "B-u1", "B-u3"]]
    assert open(os.path.join(root, "vad.scp")).read() == "left alone\n" and not [n for n in os.listdir(root) if n.endswith(".new")]
    assert filter_data_dir.filter_data_dir(root, min_len=400, min_num_utts=2) == (4, 2)      # a second pass changes nothing
    assert _read(root, "utt2spk") == [[u, spk_of[u]] for u in utts]


def test_filter_data_dir_without_rules_sorts_and_intersects(tmp_path):
    from tf_kaldi_speaker_amd.misc.tools import filter_data_dir
    frames = {"b": 3, "a": 1, "B": 2, "c": 9}
    root = str(tmp_path / "d")
    _write_dir(root, frames, {"a": "s", "b": "s", "B": "S"})      # c has no speaker
    assert filter_data_dir.filter_data_dir(root) == (3, 2)
    assert [u for u, _ in _read(root, "utt2num_frames")] == ["B", "a", "b"] and _read(root, "spk2utt") == [["S", "B"], ["s", "a", "b"]]
    # min_len is strict, min_num_utts is not
    assert filter_data_dir.filter_data_dir(root, min_len=1, min_num_utts=1) == (2, 2)
    assert [u for u, _ in _read(root, "feats.scp")] == ["B", "b"]


def test_filter_data_dir_command_line(tmp_path):
    root = str(tmp_path / "d")
    _write_dir(root, {"u1": 10, "u2": 5}, {"u1": "s", "u2": "s"})
    tool = os.path.join(PKG, "misc", "tools", "filter_data_dir.py")
    r = subprocess.run([sys.executable, tool, "--min-len", "5", root], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "keeps 1 utterances of 1 speakers" in r.stderr and _read(root, "utt2spk") == [["u1", "s"]]
    os.remove(os.path.join(root, "feats.scp"))
    r = subprocess.run([sys.executable, tool, root], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "no feats.scp" in r.stderr


def test_prepare_feats_options_are_declared_once():
    cli = _cli()
    names = ("gpu", "prep_cmn_window", "vad", "cm_header", "min_len", "write_utt2num_frames", "raw_rspecifier", "prepared_wspecifier")
    args = cli.parser_for(*names).parse_args(["ark:raw.ark", "ark,scp:out.ark,out.scp"])
    assert (args.gpu, args.cmn_window, args.vad, args.cm_header, args.min_len, args.write_utt2num_frames) == (-1, 300, "", "uniform", 0, "")
    assert (args.raw_rspecifier, args.prepared_wspecifier) == ("ark:raw.ark", "ark,scp:out.ark,out.scp")
    args = cli.parser_for(*names).parse_args(["-g", "2", "--cmn-window", "0", "--vad", "scp:vad.scp", "--cm-header", "quartiles", "--min-len", "400",
                                              "--write-utt2num-frames", "n", "ark:a", "ark:b"])
    assert (args.gpu, args.cmn_window, args.vad, args.cm_header, args.min_len, args.write_utt2num_frames) == (2, 0, "scp:vad.scp", "quartiles", 400, "n")
    for bad in (["--cm-header", "deciles", "ark:a", "ark:b"], ["--norm-vars=true", "ark:a", "ark:b"], ["--center=false", "ark:a", "ark:b"], ["ark:a"]):
        with pytest.raises(SystemExit):      # the options of apply-cmvn-sliding that are not implemented are not options: refused by name
            cli.parser_for(*names).parse_args(bad)
    assert cli.parser_for("cmn_window").parse_args([]).cmn_window == 0      # extract.py's default stays


def test_table_writer_refuses_a_wspecifier_without_ark(tmp_path):
    cli = _cli()
    for bad in ("scp:%s" % (tmp_path / "x.scp"), str(tmp_path / "x.ark"), "ark,t:%s" % (tmp_path / "x.ark"), "ark:"):
        with pytest.raises(SystemExit, match="`ark:FILE` or `ark,scp:ARK,SCP` is expected"):
            cli.Table(bad, "prepared_wspecifier")
    with pytest.raises(SystemExit, match="names 1 file\\(s\\) for 2 table type\\(s\\)"):
        cli.Table("ark,scp:%s" % (tmp_path / "x.ark"), "prepared_wspecifier")
    assert not os.listdir(str(tmp_path))
    t = cli.Table("scp,ark:%s,%s" % (tmp_path / "x.scp", tmp_path / "x.ark"), "prepared_wspecifier")
    t.write("key1", lambda fd, k: fd.write((k + " ").encode() + b"\0Bxyz"))
    t.write("k2", lambda fd, k: fd.write((k + " ").encode() + b"\0Bq"))
    t.close()
    assert open(str(tmp_path / "x.scp")).read() == "key1 %s:5\nk2 %s:13\n" % (tmp_path / "x.ark", tmp_path / "x.ark")
    assert open(str(tmp_path / "x.ark"), "rb").read()[13:] == b"\0Bq"


def test_cm_encode_offsets_and_refusals():
    """ops.cm_encode_plan: image i has 16 + 8 d + d rows[i] bytes and the images lie back to back; everything is refused before a launch."""
    from tf_kaldi_speaker_amd import ops
    rows, offsets, total, code = ops.cm_encode_plan((4, 300, 31), [1, 300, 2, 7], "quartiles")
    sizes = [16 + 8 * 31 + 31 * n for n in (1, 300, 2, 7)]
    assert rows.dtype == np.int32 and list(rows) == [1, 300, 2, 7] and offsets.dtype == np.int64
    assert list(offsets) == [0, sizes[0], sizes[0] + sizes[1], sizes[0] + sizes[1] + sizes[2]] and total == sum(sizes) and code == 0
    assert offsets[1] % 2 == 1 and list(ops.cm_image_bytes([1, 300, 2, 7], 31)) == sizes
    assert ops.cm_encode_plan((1, 5, 128), np.asarray([5]), "uniform")[2:] == (16 + 8 * 128 + 128 * 5, 1)
    # a batch beyond 2^31 bytes: the offsets are 64-bit
    big = ops.cm_encode_plan((3, 10 ** 7, 128), [10 ** 7] * 3)
    assert int(big[1][2]) == 2 * (16 + 1024 + 128 * 10 ** 7) > 2 ** 31 and big[2] == 3 * (16 + 1024 + 128 * 10 ** 7)
    with pytest.raises(IndexError, match="cm_encode: rows holds a value outside 1 .. 8"):
        ops.cm_encode_plan((2, 8, 30), [3, 0])
    with pytest.raises(IndexError, match="cm_encode: rows holds a value outside 1 .. 8"):
        ops.cm_encode_plan((2, 8, 30), [9, 3])
    with pytest.raises(ValueError, match="cm_encode: rows must be a non-empty 1-D integer array of 2"):
        ops.cm_encode_plan((2, 8, 30), [3, 3, 3])
    with pytest.raises(ValueError, match="cm_encode: rows must be"):
        ops.cm_encode_plan((2, 8, 30), [3.0, 3.0])
    with pytest.raises(ValueError, match="cm_encode: d must lie in 1 .. 128 \\(got 129\\)"):
        ops.cm_encode_plan((1, 4, 129), [4])
    with pytest.raises(ValueError, match="cm_encode: header must be 'quartiles' or 'uniform' \\(got 'deciles'\\)"):
        ops.cm_encode_plan((1, 4, 30), [4], "deciles")
