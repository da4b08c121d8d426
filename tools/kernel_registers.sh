#!/bin/bash
# VGPRs / SGPRs / spills / scratch / LDS / code size of every kernel of a translation unit as hipcc reports them (code object metadata and the
# "codeLenInByte" line behind each kernel's text; no GPU needed):
#   tools/kernel_registers.sh xv_gemm.hip [-DFLAGS...] > profiles/rNN_kernel_registers.txt
# XV_CSRC=<dir>: read the unit from another checkout's csrc directory (a before / after table of a refactor)
unit=$1; shift
R=$(cd $(dirname $0)/.. && pwd)
src=${XV_CSRC:-$R/tf_kaldi_speaker_amd/csrc}
inc=$(dirname $(dirname $src))/include
tmp=$(mktemp /tmp/xvreg.XXXX.s)
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I$inc -I$src "$@" -S --cuda-device-only $src/$unit -o $tmp 2>/dev/null || exit 1
echo "# $unit $* : hipcc -S --offload-arch=gfx950, amdhsa.kernels metadata + codeLenInByte"
printf "%-64s %6s %6s %7s %8s %7s %8s\n" kernel vgprs sgprs spilled scratchB ldsB codeB
awk '/^\t\.amdhsa_kernel /{cur=$2} /^; Kernel info:/{k=1} /^; Function info:/{k=0} k && /^; codeLenInByte = /{len[cur]=$4; k=0}
     /^amdhsa.kernels:/{on=1} on && /\.group_segment_fixed_size:/{lds=$2} on && /\.name:/{name=$2} on && /\.private_segment_fixed_size:/{scr=$2}
     on && /\.sgpr_count:/{sg=$2} on && /\.vgpr_count:/{v=$2} on && /\.vgpr_spill_count:/{print name, v, sg, $2, scr, lds, len[name]}' $tmp |
  while read n v g s c l b; do printf "%-64s %6s %6s %7s %8s %7s %8s\n" "$(echo $n | c++filt | cut -c1-64)" $v $g $s $c $l $b; done
rm -f $tmp
