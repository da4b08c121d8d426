#!/usr/bin/env python3
"""Log-mel filterbank features, and optionally energy VAD decisions, from a wav.scp on the GPU:

    python nnet/lib/make_fbank.py [-g GPU] [--fbank-config conf/fbank.conf] [--vad-config conf/vad.conf] [--compress {true,false}]
                                  [--write-utt2num-frames FILE]
                                  [--augment-plan PLAN --rir-scp F --noise-scp F [--augment-config conf] [--resample-signals true]]
                                  wav.scp ark,scp:feats.ark,feats.scp [ark,scp:vad.ark,vad.scp]

What steps/make_fbank.sh --fbank-config conf/fbank.conf does (compute-fbank-feats | copy-feats --compress=true), with --dither=0; the
kernel is xv_fbank (include/xvector_hip.h), the MFCC kernel stopped in front of the DCT.  This is make_mfcc.py's program - its reader, its
rate rules (--allow-downsample / --allow-upsample in the conf), --compress, --write-utt2num-frames and --augment-plan are that module's
code, not a copy - with two differences: the conf is compute-fbank-feats' (misc.features.FbankOptions: its own defaults, 23 bins, snip-edges
true; --use-log-fbank, --use-power; what is not implemented is refused by name), and the VAD wspecifier may be left out.  When it is given,
the decisions come from the log-energy xv_fbank computes beside the features (energy_out), whatever --use-energy says: they are the
decisions make_mfcc.py writes for an MFCC conf with the same framing and --use-energy=true, without the second feature pass Kaldi recipes
run for the VAD of a filterbank system.
"""
import make_mfcc

if __name__ == "__main__":
    make_mfcc.main("fbank")
