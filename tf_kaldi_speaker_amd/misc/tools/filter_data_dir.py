#!/usr/bin/env python3
"""The bookkeeping of stage 5 of the recipe (egs/voxceleb/v1/run.sh:140-163) on a Kaldi data directory, without Kaldi's utils/:

    python filter_data_dir.py [--min-len N] [--min-num-utts M] data_dir

Rewrites utt2num_frames, utt2spk, spk2utt and feats.scp of data_dir so that they list the same utterances, sorted by key in C order
(what utils/fix_data_dir.sh leaves).  An utterance stays if it is in utt2num_frames, utt2spk and feats.scp, has frames > N
(awk '$2 > min_len') and - counted after that - its speaker keeps at least M utterances (awk '$2 >= min_num_utts' on spk2num).
spk2utt is derived from utt2spk; other files of the directory are not touched.  Host only.
"""
import argparse
import os
import sys


def read_table(path):
    """{key: the rest of the line} of a `key value...` file, in file order."""
    out = {}
    with open(path, "r") as f:
        for line in f:
            fields = line.strip().split(None, 1)
            if fields:
                out[fields[0]] = fields[1] if len(fields) > 1 else ""
    return out


def filter_tables(utt2num_frames, utt2spk, feats, min_len=0, min_num_utts=0):
    """The three tables ({utt: frames}, {utt: speaker}, {utt: rxfilename}) -> (the utterances kept, sorted; {speaker: its kept
    utterances, sorted}, the speakers in sorted order too)."""
    utts = [u for u in utt2num_frames if u in utt2spk and u in feats and int(utt2num_frames[u]) > min_len]
    spk2utt = {}
    for u in sorted(utts):
        spk2utt.setdefault(utt2spk[u], []).append(u)
    spk2utt = {s: spk2utt[s] for s in sorted(spk2utt) if len(spk2utt[s]) >= min_num_utts}
    return sorted(u for us in spk2utt.values() for u in us), spk2utt


def filter_data_dir(data_dir, min_len=0, min_num_utts=0):
    """-> (utterances kept, speakers kept) after rewriting the four files."""
    path = lambda name: os.path.join(data_dir, name)
    for name in ("utt2num_frames", "utt2spk", "feats.scp"):
        if not os.path.isfile(path(name)):
            raise ValueError("%s: no %s" % (data_dir, name))
    frames, utt2spk, feats = read_table(path("utt2num_frames")), read_table(path("utt2spk")), read_table(path("feats.scp"))
    utts, spk2utt = filter_tables(frames, utt2spk, feats, min_len, min_num_utts)
    for name, lines in (("utt2num_frames", ["%s %s" % (u, frames[u]) for u in utts]), ("utt2spk", ["%s %s" % (u, utt2spk[u]) for u in utts]),
                        ("feats.scp", ["%s %s" % (u, feats[u]) for u in utts]), ("spk2utt", [" ".join([s] + us) for s, us in spk2utt.items()])):
        with open(path(name) + ".new", "w") as f:
            f.write("".join(line + "\n" for line in lines))
        os.replace(path(name) + ".new", path(name))
    return len(utts), len(spk2utt)


def main(argv=None):
    ap = argparse.ArgumentParser(usage="%(prog)s [--min-len N] [--min-num-utts M] data_dir")
    ap.add_argument("--min-len", type=int, default=0, help="Keep utterances with frames > N (the recipe: 400).")
    ap.add_argument("--min-num-utts", type=int, default=0, help="Keep speakers with at least M remaining utterances (the recipe: 8).")
    ap.add_argument("data_dir")
    args = ap.parse_args(argv)
    try:
        utts, spks = filter_data_dir(args.data_dir, args.min_len, args.min_num_utts)
    except ValueError as e:
        sys.exit(str(e))
    sys.stderr.write("filter_data_dir: %s keeps %d utterances of %d speakers\n" % (args.data_dir, utts, spks))


if __name__ == "__main__":
    main()
