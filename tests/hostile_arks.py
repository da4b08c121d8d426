"""Arks and data directories no well-meaning tool writes, for the shipped libxvector_io.so (tests/test_native_loader.py): the corpus of
tests/host_san/loader_san.cpp's `hostile` scenario, restated in Python.  Run as a program it writes the corpus under a directory, takes
every entry through nl.read_rows and through NativeRandomQueue.start() / fetch(), and prints one JSON list of the entries that were
not refused as expected - in a process of its own, so that a wild copy ends this program and not the test run.

    python tests/hostile_arks.py <directory>            (XVIO_NO_MMAP in the environment selects the pread path)
"""
import io
import json
import os
import struct
import sys

import numpy as np

I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
BAD, SMALL, CUT, NOHEAD, NOTBIN = "shape", "output buffer too small", "truncated", "cannot read the matrix header", "not a binary Kaldi object"
NOT_ENOUGH = "The number of frames is not enough"


def plain_header(kind, rows, cols):
    return b"\0B" + kind + b"M \x04" + struct.pack("<i", rows) + b"\x04" + struct.pack("<i", cols)


def cm_header(rows, cols):
    return b"\0BCM " + struct.pack("<ffii", 0.0, 1.0, rows, cols)


def matrix(kind, rows, cols, seed):
    """(bytes of a well-formed matrix from its marker, bytes of its header region)"""
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    m = np.random.RandomState(seed).randn(rows, cols)
    f = io.BytesIO()
    if kind == b"C":
        kaldi_io.write_compressed_mat(f, m.astype(np.float32))
        return f.getvalue(), 5 + 16 + 8 * cols
    kaldi_io.write_mat(f, m.astype(np.float32 if kind == b"F" else np.float64))
    return f.getvalue(), 15


def entries():
    """dicts: name, ark (bytes), offset, rr / ld (message of read_rows / of the loader, None = not read that way), frames, T, segments,
    packed (also through a packed loader), names (what the message must name, None = the ark), second (offset of a second utterance)"""
    def e(name, ark, offset=4, rr=None, ld=None, frames=10, T=4, segments=1, packed=False, names=None, second=None):
        return dict(name=name, ark=ark, offset=offset, rr=rr, ld=ld, frames=frames, T=T, segments=segments, packed=packed, names=names, second=second)
    out = []
    for k in (b"F", b"D"):
        kn = k.decode() + "M"
        for rows, cols, rr, ld in [(10, -3, BAD, BAD), (10, -1, BAD, BAD), (10, 0, BAD, BAD), (10, I32_MIN, BAD, BAD), (-1, 5, BAD, BAD),
                                   (0, 5, BAD, BAD), (I32_MIN, 5, BAD, BAD), (10, I32_MAX, SMALL, SMALL), (I32_MAX, 5, SMALL, CUT),
                                   (65536, 65536, SMALL, CUT), (46341, 46341, SMALL, CUT), (I32_MAX, 2, SMALL, CUT),
                                   (I32_MAX, I32_MAX, BAD, BAD), (I32_MIN, I32_MIN, BAD, BAD), (-1, -1, BAD, BAD)]:
            out.append(e("%s %d x %d" % (kn, rows, cols), b"key " + plain_header(k, rows, cols) + b"xxx", rr=rr, ld=ld))
    for rows, cols, rr, ld in [(0, 5, BAD, BAD), (-1, 5, BAD, BAD), (5, 0, BAD, BAD), (5, -2, BAD, BAD), (I32_MIN, I32_MIN, BAD, BAD),
                               (10, I32_MAX, SMALL, SMALL), (I32_MAX, 5, SMALL, CUT), (I32_MAX, I32_MAX, SMALL, SMALL)]:
        out.append(e("CM %d x %d" % (rows, cols), b"key " + cm_header(rows, cols) + b"x" * 96, rr=rr, ld=ld))
    fm, _ = matrix(b"F", 6, 5, 1)
    for marker in (b"\0C", b"AB", b"B\0"):
        out.append(e("marker %r" % marker, b"key " + marker + fm[2:], rr=NOTBIN, ld=NOTBIN))
    for kind in (b"XM ", b"HM ", b"FV "):
        want = "The header contained '%s'" % kind.decode()
        out.append(e("kind %r" % kind, b"key \0B" + kind + fm[5:], rr=want, ld=want))
    # every cut from the marker to 16 bytes past the header region, then the middle of the data and one and two bytes short of the last
    # byte of rows [0, rows-1) (the longest chunk a loader draws from `rows` frames); the whole matrix less one byte for read_rows
    for k in (b"C", b"F", b"D"):
        blob, hdr = matrix(k, 6, 5, 2)
        total, data = len(blob), len(blob) - hdr
        read_end = total - 1 if k == b"C" else total - data // 6
        for n in list(range(hdr + 17)) + [hdr + 16 + (data - 16) // 2, read_end - 2, read_end - 1]:
            want = NOHEAD if n < 5 else CUT
            out.append(e("%sM 6x5 cut after %d of %d bytes" % (k.decode(), n, total), b"key " + blob[:n], rr=want, ld=want, frames=6, T=5, packed=k == b"C"))
        out.append(e("%sM 6x5 without its last byte" % k.decode(), b"key " + blob[:-1], rr=CUT))
    cm, _ = matrix(b"C", 20, 5, 3)
    good = b"key " + cm
    out.append(e("offset -1", good, offset=-1, rr=NOHEAD, ld=NOHEAD))
    out.append(e("offset 0 (the key text)", good, offset=0, rr=NOTBIN, ld=NOTBIN))
    out.append(e("offset = file size", good, offset=len(good), rr=NOHEAD, ld=NOHEAD))
    out.append(e("offset = file size - 1", good, offset=len(good) - 1, rr=NOHEAD, ld=NOHEAD))
    out.append(e("utt2num_frames claims 1000 rows of 20", good, ld=NOT_ENOUGH, frames=1000, T=50, packed=True))
    out.append(e("utt2num_frames claims 21 rows of 20", good, ld=NOT_ENOUGH, frames=21, T=20, packed=True))
    out.append(e("utt2num_frames 0", good, ld="has 0 frames", frames=0, names="utt2num_frames"))
    out.append(e("utt2num_frames -5", good, ld="has -5 frames", frames=-5, names="utt2num_frames"))
    for k in (b"C", b"F", b"D"):
        for cols2 in (3, 7):
            two = b"u1 " + matrix(k, 30, 5, 4)[0] + b"u2 "
            out.append(e("%sM 5 columns, then %d" % (k.decode(), cols2), two + matrix(k, 30, cols2, 5)[0], offset=3, ld="feature dimension changes",
                         frames=30, T=10, segments=2, packed=k == b"C", second=len(two)))
    return out


def run(root):
    """[(entry name, reader, what happened)] for every entry that was not refused with its message"""
    from tf_kaldi_speaker_amd.dataset import native_loader as nl
    nl.load()
    wrong = []
    for i, en in enumerate(entries()):
        ark, d = os.path.join(root, "h%d.ark" % i), os.path.join(root, "h%d.d" % i)
        with open(ark, "wb") as f:
            f.write(en["ark"])
        names = en["names"] or ark

        def check(reader, fragment, call):
            try:
                call()
            except nl.XvioError as err:
                if fragment not in str(err) or names not in str(err):
                    wrong.append((en["name"], reader, "refused with %r, expected %r naming %s" % (str(err), fragment, names)))
            else:
                wrong.append((en["name"], reader, "accepted, expected %r" % fragment))

        if en["rr"] is not None:
            check("read_rows", en["rr"], lambda: nl.read_rows(ark, en["offset"], max_elems=1 << 16))
        if en["ld"] is None:
            continue
        os.makedirs(d)
        utts = [("s1-u1", en["offset"])] + ([("s1-u2", en["second"])] if en["second"] is not None else [])
        with open(os.path.join(d, "feats.scp"), "w") as f:
            f.write("".join("%s %s:%d\n" % (u, ark, off) for u, off in utts))
        with open(os.path.join(d, "spk2utt"), "w") as f:
            f.write("s1 %s\n" % " ".join(u for u, _ in utts))
        with open(os.path.join(d, "utt2num_frames"), "w") as f:
            f.write("".join("%s %d\n" % (u, en["frames"]) for u, _ in utts))
        with open(os.path.join(d, "spklist"), "w") as f:
            f.write("s1 0\n")
        for packed in ([False, True] if en["packed"] else [False]):
            def through_the_loader():
                q = nl.NativeRandomQueue(d, os.path.join(d, "spklist"), num_parallel=1, max_qsize=1, num_speakers=1, num_segments=en["segments"],
                                         min_len=en["T"], max_len=en["T"], shuffle=False, seed=1, packed=packed)
                try:
                    q.start()
                    if q.dim <= 0:
                        wrong.append((en["name"], "loader", "a loader with dim %d" % q.dim))
                        raise nl.XvioError("%s %s" % (en["ld"], names))
                    q.fetch()
                finally:
                    q.stop()
            check("packed loader" if packed else "loader", en["ld"], through_the_loader)
    return wrong


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("HOSTILE " + json.dumps(run(sys.argv[1])))
