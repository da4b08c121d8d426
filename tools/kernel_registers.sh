#!/bin/bash
# VGPRs / SGPRs / spills / scratch / LDS / code size of every kernel of a translation unit as hipcc reports them (code object metadata and the
# "codeLenInByte" line behind each kernel's text; no GPU needed), and a hash of each kernel's instruction stream:
#   tools/kernel_registers.sh xv_gemm_nt.hip [-DFLAGS...] > profiles/rNN_kernel_registers.txt
# XV_CSRC=<dir>: read the unit from another checkout's csrc directory (a before / after table of a refactor)
# isa16 = the first 16 hex digits of the sha256 of the kernel's disassembly (llvm-objdump -d of the device ELF, symbol by symbol, cut at the
# symbol's size): one line per instruction, "mnemonic operands | encoding words", without the address column - branch encodings are relative,
# so the hash does not depend on where the kernel sits in the code object.  Equal hashes and equal columns = the same kernel.
unit=$1; shift
R=$(cd $(dirname $0)/.. && pwd)
src=${XV_CSRC:-$R/tf_kaldi_speaker_amd/csrc}
inc=$(dirname $(dirname $src))/include
llvm=${ROCM_PATH:-/opt/rocm}/llvm/bin
tmp=$(mktemp /tmp/xvreg.XXXX.s)
isa=$(mktemp -d /tmp/xvisa.XXXX)
FL="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -I$inc -I$src"
hipcc $FL "$@" -S --cuda-device-only $src/$unit -o $tmp 2>/dev/null || exit 1
hipcc $FL "$@" --offload-device-only --no-gpu-bundle-output -c $src/$unit -o $isa/unit.elf 2>/dev/null || exit 1
$llvm/llvm-readelf -sW $isa/unit.elf | awk '$4 == "FUNC" {print $8, $3}' > $isa/sizes
$llvm/llvm-objdump -d $isa/unit.elf | awk -v dir=$isa '
    FNR == NR {size[$1] = $2; next}
    /^[0-9a-f]+ <.*>:$/ {cur = substr($2, 2, length($2) - 3); left = size[cur]; next}
    cur != "" && left > 0 && / \/\/ [0-9A-F]+: / {
        split($0, h, " // "); text = h[1]; sub(/^[ \t]+/, "", text); sub(/[ \t]+$/, "", text)
        n = split(h[2], w, " "); enc = ""
        for (i = 2; i <= n && w[i] ~ /^[0-9A-F]+$/ && length(w[i]) == 8; ++i) {enc = enc " " w[i]; left -= 4}
        print text " |" enc > (dir "/" cur ".isa")
    }' $isa/sizes -
echo "# $unit $* : hipcc -S --offload-arch=gfx950, amdhsa.kernels metadata + codeLenInByte; isa16: sha256 of llvm-objdump -d without addresses"
printf "%-64s %6s %6s %7s %8s %7s %8s %17s\n" kernel vgprs sgprs spilled scratchB ldsB codeB isa16
awk '/^\t\.amdhsa_kernel /{cur=$2} /^; Kernel info:/{k=1} /^; Function info:/{k=0} k && /^; codeLenInByte = /{len[cur]=$4; k=0}
     /^amdhsa.kernels:/{on=1} on && /\.group_segment_fixed_size:/{lds=$2} on && /\.name:/{name=$2} on && /\.private_segment_fixed_size:/{scr=$2}
     on && /\.sgpr_count:/{sg=$2} on && /\.sgpr_spill_count:/{ss=$2} on && /\.vgpr_count:/{v=$2}
     on && /\.vgpr_spill_count:/{print name, v, sg, $2 "/" ss, scr, lds, len[name]}' $tmp |
  while read n v g s c l b; do
    printf "%-64s %6s %6s %7s %8s %7s %8s %17s\n" "$(echo $n | c++filt | cut -c1-64)" $v $g $s $c $l $b $(sha256sum < $isa/$n.isa | cut -c1-16)
  done
[ -n "$XV_ISA_KEEP" ] && mkdir -p $XV_ISA_KEEP && cp $isa/*.isa $XV_ISA_KEEP/      # XV_ISA_KEEP=<dir>: keep the normalised streams (diff them)
rm -rf $tmp $isa
