"""libxvector_io.so (the native Kaldi loader) on the CPU: ABI vs include/xvector_io.h, the 'CM ' sub-range codec bit-exact
against the Python reader (which tests/test_host_io.py pins against the reference's kaldi_io through tests/golden), the
reference's sampling rules, determinism in (seed, batch index) for any thread count, error behaviour."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.kaldi_fixture import make_data_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xvector_io.h")


@pytest.fixture(scope="module")
def nl():
    from tf_kaldi_speaker_amd.dataset import native_loader
    native_loader.load()
    return native_loader


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kaldi_native"))
    return make_data_dir(root, num_spk=8, utts_per_spk=4, dim=30, min_frames=70, max_frames=160, seed=3)


def test_abi_matches_header(nl):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(xvio_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(nl.SIGNATURES)
    lib = ctypes.CDLL(nl.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), "libxvector_io.so does not export %s" % n
    assert nl.load().xvio_abi_version() == 2
    body = src[src.index("typedef struct xvio_config {") + len("typedef struct xvio_config {"):src.index("} xvio_config;")]
    fields = []
    for line in body.split(";"):
        m = re.match(r"\s*(const char\*|int32_t|uint64_t)\s+(.+)", line.strip(), flags=re.S)
        if m:
            fields += [(m.group(1), nm.strip()) for nm in m.group(2).split(",")]
    kinds = {ctypes.c_char_p: "const char*", ctypes.c_int32: "int32_t", ctypes.c_uint64: "uint64_t"}
    assert fields == [(kinds[t], n) for n, t in nl.XvioConfig._fields_]


def _scp(root):
    out = {}
    for line in open(os.path.join(root, "feats.scp")):
        utt, rx = line.strip().split(" ", 1)
        path, off = rx.rsplit(":", 1)
        out[utt] = (path, int(off))
    return out


def test_cm_rows_bit_exact_with_python_reader(nl, data):
    from tf_kaldi_speaker_amd.dataset.kaldi_io import FeatureReader
    root, spklist, mats = data
    reader = FeatureReader(root)
    scp = _scp(root)
    rs = np.random.RandomState(0)
    for utt, (path, off) in list(scp.items())[:12]:
        n = mats[utt].shape[0]
        whole = nl.read_rows(path, off)
        ref, _ = reader.read("%s %s:%d" % (utt, path, off))
        assert whole.shape == (n, 30) and np.array_equal(whole, ref)
        for _ in range(3):
            length = int(rs.randint(1, n + 1))
            start = int(rs.randint(0, n - length + 1))
            seg = nl.read_rows(path, off, start, length)
            ref, _ = reader.read_segment("%s %s:%d" % (utt, path, off), length, start=start)
            assert np.array_equal(seg, ref), (utt, start, length)
        assert np.abs(whole - mats[utt]).max() < 0.05          # the codec is lossy: sanity only
    reader.close()


def test_fm_and_dm_matrices(nl, tmp_path):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    rs = np.random.RandomState(1)
    for dt in (np.float32, np.float64):
        m = rs.randn(37, 24).astype(dt)
        path = str(tmp_path / ("m_%s.ark" % np.dtype(dt).name))
        with open(path, "wb") as f:
            f.write(b"key ")
            off = f.tell()
            kaldi_io.write_mat(f, m)
        assert np.array_equal(nl.read_rows(path, off), m.astype(np.float32))
        assert np.array_equal(nl.read_rows(path, off, 5, 11), m[5:16].astype(np.float32))


def test_errors_are_reported(nl, data, tmp_path):
    root, spklist, _ = data
    path, off = next(iter(_scp(root).values()))
    with pytest.raises(nl.XvioError, match="not enough"):
        nl.read_rows(path, off, 0, 100000)
    with pytest.raises(nl.XvioError, match="cannot open"):
        nl.read_rows(str(tmp_path / "missing.ark"), 0)
    with pytest.raises(nl.XvioError, match="not a binary Kaldi object"):
        nl.read_rows(path, off + 1)
    q = nl.NativeRandomQueue(str(tmp_path), spklist, num_speakers=2, num_segments=2, min_len=10, max_len=20)
    with pytest.raises(nl.XvioError, match="cannot open"):
        q.start()
    q = nl.NativeRandomQueue(root, spklist, num_speakers=4, num_segments=2, min_len=1000, max_len=1200, seed=1)
    q.start()
    with pytest.raises(nl.XvioError, match="longer than"):      # no utterance is that long: reported, not hung
        q.fetch()
    q.stop()


def test_pread_path_without_mmap(nl, data, tmp_path, monkeypatch):
    """XVIO_NO_MMAP=1 (include/xvector_io.h): no mapping, every read through pread - same rows bit for bit, and an ark that was cut
    short after it was indexed is a clean error, not a SIGBUS."""
    import shutil
    root, spklist, mats = data
    scp = _scp(root)
    utt, (path, off) = list(scp.items())[-1]              # a matrix near the end of its ark
    want = nl.read_rows(path, off)
    monkeypatch.setenv("XVIO_NO_MMAP", "1")
    assert np.array_equal(nl.read_rows(path, off), want)
    assert np.array_equal(nl.read_rows(path, off, 3, 20), want[3:23])
    out, _ = _collect(nl, root, spklist, 2, 3)
    monkeypatch.delenv("XVIO_NO_MMAP")
    ref, _ = _collect(nl, root, spklist, 2, 3)
    for (f, l), (g, m) in zip(out, ref):
        assert np.array_equal(f, g) and np.array_equal(l, m)
    monkeypatch.setenv("XVIO_NO_MMAP", "1")
    cut = str(tmp_path / "cut.ark")
    shutil.copyfile(path, cut)
    with open(cut, "r+b") as fh:
        fh.truncate(off + 40)                             # header and a few column headers survive, the data do not
    with pytest.raises(nl.XvioError, match="truncated"):
        nl.read_rows(cut, off)


def _collect(nl, root, spklist, threads, n, seed=11, **kw):
    args = dict(num_speakers=5, num_segments=3, min_len=40, max_len=65, shuffle=True)
    args.update(kw)
    q = nl.NativeRandomQueue(root, spklist, num_parallel=threads, max_qsize=4, seed=seed, **args)
    q.start()
    out = [q.fetch() for _ in range(n)]
    stats = q.stats()
    q.stop()
    return out, stats


def test_batches_follow_the_reference_sampling_rules(nl, data):
    root, spklist, mats = data
    spk_of = {int(l.split()[1]): l.split()[0] for l in open(spklist)}
    decoded = {utt: nl.read_rows(*_scp(root)[utt]) for utt in mats}
    batches, (nb, sec) = _collect(nl, root, spklist, threads=3, n=12)
    assert nb >= 12 and sec > 0
    lengths = set()
    for feats, labels in batches:
        b, t, d = feats.shape
        assert b == 15 and d == 30 and 40 <= t <= 65 and labels.shape == (15,) and labels.dtype == np.int32
        lengths.add(t)
        per_spk = labels.reshape(5, 3)
        assert np.all(per_spk == per_spk[:, :1])                       # num_segments consecutive chunks per speaker
        assert len(set(per_spk[:, 0])) == 5                            # distinct speakers within a batch
        for i in range(b):
            spk = spk_of[int(labels[i])]
            hit = False
            for utt, m in decoded.items():                             # the chunk is T consecutive rows of one utterance of that speaker
                if not utt.startswith(spk) or m.shape[0] <= t:
                    continue
                for s in np.nonzero(np.all(m[:m.shape[0] - t + 1] == feats[i, 0], axis=1))[0]:
                    if np.array_equal(m[s:s + t], feats[i]):
                        hit = True
            assert hit, "row %d of the batch is not a window of an utterance of %s" % (i, spk)
    assert len(lengths) > 3                                            # one T per batch, varying between batches


def test_stream_is_a_function_of_seed_and_index_only(nl, data):
    root, spklist, _ = data
    a, _ = _collect(nl, root, spklist, threads=1, n=10)
    b, _ = _collect(nl, root, spklist, threads=4, n=10)
    for (fa, la), (fb, lb) in zip(a, b):
        assert np.array_equal(fa, fb) and np.array_equal(la, lb)
    c, _ = _collect(nl, root, spklist, threads=2, n=3, seed=12)
    assert not all(np.array_equal(x[1], y[1]) and x[0].shape == y[0].shape for x, y in zip(a, c))


def test_packed_batches_decode_to_the_host_decoded_ones(nl, data, tmp_path):
    """xvio_config.packed: the threads deliver the rows' undecoded 'CM ' pieces (for xv_cm_decode on the GPU).  Decoded with the NumPy
    restatement of that kernel, batch i is bit-identical to batch i of the host-decoding loader with the same seed - odd lengths (a
    chunk stride that needs its 16-byte padding) included; FM / DM data is refused by name."""
    root, spklist, _ = data
    a, _ = _collect(nl, root, spklist, threads=2, n=8)
    b, _ = _collect(nl, root, spklist, threads=3, n=8, packed=True)
    assert {x[0].shape[1] % 2 for x in a} == {0, 1}
    for (fa, la), (fb, lb) in zip(a, b):
        assert fa.shape == fb.shape and fb.dtype == np.float32
        assert np.array_equal(fa, fb) and np.array_equal(la, lb)
    assert nl.packed_chunk_bytes(30, 41) == (8 + 240 + 30 * 41 + 15) // 16 * 16
    # an uncompressed ark: the packed loader says what it needs instead of decoding garbage
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    d = tmp_path / "fm"
    d.mkdir()
    with open(d / "feats.ark", "wb") as f:
        f.write(b"s1-u1 ")
        off = f.tell()
        kaldi_io.write_mat(f, np.random.RandomState(0).randn(90, 30).astype(np.float32))
    (d / "feats.scp").write_text("s1-u1 %s:%d\n" % (d / "feats.ark", off))
    (d / "spk2utt").write_text("s1 s1-u1\n")
    (d / "utt2num_frames").write_text("s1-u1 90\n")
    (d / "spklist").write_text("s1 0\n")
    q = nl.NativeRandomQueue(str(d), str(d / "spklist"), num_parallel=1, max_qsize=2, num_speakers=1, num_segments=1, min_len=40, max_len=50, seed=1,
                             packed=True)
    q.start()
    with pytest.raises(nl.XvioError, match="needs 'CM ' compressed matrices"):
        q.fetch()
    q.stop()
    plain = nl.NativeRandomQueue(str(d), str(d / "spklist"), num_parallel=1, max_qsize=2, num_speakers=1, num_segments=1, min_len=40, max_len=50, seed=1)
    plain.start()
    assert plain.fetch()[0].shape[2] == 30
    plain.stop()


def test_packed_bytes_do_not_depend_on_the_ring_depth(nl, data):
    """Batch i is a function of (seed, i) down to its raw bytes: a packed chunk's padding (up to 15 bytes of its 16-byte stride) is
    zero, not whatever an earlier batch of another length left in the ring slot - the bytes are the same for every max_qsize."""
    root, spklist, _ = data
    streams, pads = {}, 0
    for depth in (1, 2, 5):
        q = nl.NativeRandomQueue(root, spklist, num_parallel=2, max_qsize=depth, seed=11, num_speakers=5, num_segments=3, min_len=40, max_len=65,
                                 shuffle=True, packed=True)
        q.start()
        out = []
        for _ in range(12):
            buf, lab = np.full(15 * nl.packed_chunk_bytes(q.dim, 65), 0xA5, np.uint8), np.empty(15, np.int32)
            t = q.fetch_packed_into(buf, lab)
            stride, used = nl.packed_chunk_bytes(q.dim, t), 8 + 8 * q.dim + q.dim * t
            raw = buf[:15 * stride].reshape(15, stride)
            assert not raw[:, used:].any(), "depth %d: padding bytes of a %d-frame batch are not zero" % (depth, t)
            pads += stride - used
            out.append((t, raw.tobytes(), lab.tobytes()))
        q.stop()
        streams[depth] = out
    assert pads > 0                                                    # the lengths drawn leave padding to compare
    assert streams[1] == streams[2] == streams[5]


@pytest.mark.parametrize("mapped", [True, False], ids=["mapped", "pread"])
def test_hostile_arks_are_refused_by_the_shipped_library(mapped, tmp_path):
    """tests/hostile_arks.py: headers with negative, zero and overflowing shapes, foreign markers, every truncation of a small matrix,
    scp offsets off the matrix, utt2num_frames above the matrix and below 1, a second utterance with other columns.  The release build
    refuses each by name through read_rows and through start() / fetch(), mapping on and off, as the instrumented build does
    (tests/test_loader_sanitized.py) - in a child process, whose crash is this test's failure and not the run's end."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k != "XVIO_NO_MMAP"}
    if not mapped:
        env["XVIO_NO_MMAP"] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hostile_arks.py"), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, env=env, timeout=120)
    assert p.returncode == 0, "the child ended with status %d:\n%s" % (p.returncode, p.stderr[-3000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("HOSTILE ")]
    assert len(lines) == 1, p.stdout[-2000:]
    assert json.loads(lines[0][len("HOSTILE "):]) == []


def test_no_shuffle_starts_at_frame_zero_and_few_speakers_are_duplicated(nl, data):
    root, spklist, mats = data
    decoded = {utt: nl.read_rows(*_scp(root)[utt]) for utt in mats}
    batches, _ = _collect(nl, root, spklist, threads=2, n=3, shuffle=False, num_speakers=12, num_segments=2, min_len=30, max_len=30)
    for feats, labels in batches:
        assert feats.shape == (24, 30, 30)
        for i in range(24):
            assert any(np.array_equal(m[:30], feats[i]) for m in decoded.values())


def _usable_cpus():
    """CPUs this process may run on: the affinity mask, capped by the cgroup's CPU quota (os.cpu_count() is the whole machine's count)"""
    import os
    import sys
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from bench import cgroup_cpus
    quota = cgroup_cpus()
    return max(1, min(n, int(quota)) if quota else n)


def test_concurrent_loaders_scale_with_the_usable_cpus(tmp_path):
    """One native loader per rank, as an 8-GPU job runs them (tools/bench_host.py loader_scale): the instances share nothing but the page
    cache, so up to 8 single-threaded loaders in as many processes must deliver close to that many times one of them when the host has
    the cores (no global lock, no shared queue) - the property the >= 6x 1 -> 8 GPU scaling target rests on.  The
    absolute figure against the per-GPU step rate is printed by the tool on the GPU box's host (profiles/).
    A loader keeps one CPU busy, so the loader count is the CPUs this process may use (affinity and cgroup quota), at most 8.  Rates are
    the best of three interleaved rounds with timed windows of about a second: another process's burst on a shared host lowers a
    throughput sample and never raises one, so the best sample is the capability the bound is about."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import bench_host
    root, spklist, _ = make_data_dir(str(tmp_path / "d"), num_spk=40, utts_per_spk=4, dim=30, min_frames=450, max_frames=600, seed=3)
    procs = min(8, _usable_cpus())
    ones, manys = [], []
    for _ in range(3):
        ones.append(bench_host.loader_scale_run(1, 1, 500, chunks=32, root=root, spklist=spklist))
        manys.append(bench_host.loader_scale_run(procs, 1, 500, chunks=32, root=root, spklist=spklist))
    one = max(ones, key=lambda r: r["aggregate_chunks_per_s"])
    many = max(manys, key=lambda r: r["aggregate_chunks_per_s"])
    print("one loader %.0f chunks/s, %d loaders %.0f chunks/s aggregate (best of 3)" % (one["aggregate_chunks_per_s"], procs,
                                                                                        many["aggregate_chunks_per_s"]))
    assert many["aggregate_chunks_per_s"] >= 0.35 * procs * one["aggregate_chunks_per_s"], (ones, manys)
