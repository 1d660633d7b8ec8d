#!/bin/bash
# Builds timing-ablation variants of the library (here, no GPU): tools/ab/lib_mx_<name>.so from a temporary copy of the sources whose
# slab bodies of k_trunk_mx_c128 are generated with knobs (tools/gen_tower_asm.py --ablate / --dma-place / --body-pad).  Results of the
# ablated variants are WRONG on purpose; only their launch time means anything.
#   usage: tools/experiments/mx_ablate.sh name=spec ...      e.g.  nobarrier=nobarrier noc=noc,nohi dmaB0=place:B0 pad=pad:all t=define:MX_TIMING
#   mx2 / mx2:<DEFINE> / mx12 / mx12:<DEFINE> / place2:<B|BC> / ablate2:<nodma,nobarrier>: a library that also holds a variant that was measured and not adopted,
#   k_trunk_mx2_c128 or k_trunk_mx12_c128 (cz_trunk_mx2.h, cz_trunk_mx12.h; run with CCHESS_MX_KERNEL=2 / 12): the copy gets their
#   headers, their generated bodies (gen_experiments_asm.py; not kept in git) and their launch hook (patches/mx_variants_hook.patch),
#   e.g.  mx2=mx2  timing=mx2:MX2_TIMING  noxch=mx2:MX2_ABLATE_NO_EXCHANGE  dmaBC=place2:BC  mx12=mx12
# On the GPU box:  for l in tools/ab/lib_mx_*.so; do CCHESS_HIP_LIB=$(realpath $l) python tools/mx_check.py --blocks "" --time --engines mx; done
set -e
cd "$(dirname "$0")/../.."
mkdir -p tools/ab
SOURCES=$(python3 -c "import sys; sys.path.insert(0, 'cchess_zero_amd'); import build; print(' '.join(build.SOURCES))")   # the library's own list
variant() {   # the copy in $top becomes an experiment build: $1 = the experiments generator's options
  cp tools/experiments/cz_trunk_mx2.h tools/experiments/cz_trunk_mx12.h $d/
  python3 tools/experiments/gen_experiments_asm.py $d $1 > /dev/null
  patch -p1 -s -F0 -d $top < tools/experiments/patches/mx_variants_hook.patch
}
for spec in "$@"; do
  name=${spec%%=*}; flags=${spec#*=}
  top=$(mktemp -d /tmp/mxab.XXXX); d=$top/cchess_zero_amd/csrc; mkdir -p $d $top/include
  cp -r cchess_zero_amd/csrc/. $d/; cp include/cchess_hip.h $top/include/
  DEF=""; GEN=""
  case $flags in place:*) GEN="--dma-place ${flags#place:}";;
                 pad:*) GEN="--body-pad ${flags#pad:}";;
                 place2:*) DEF="-DCZ_EXPERIMENT_MX2"; variant "--dma-place2 ${flags#place2:}";;
                 ablate2:*) DEF="-DCZ_EXPERIMENT_MX2"; variant "--ablate ${flags#ablate2:}";;
                 mx2) DEF="-DCZ_EXPERIMENT_MX2"; variant;;
                 mx12) DEF="-DCZ_EXPERIMENT_MX12"; variant;;
                 mx12:*) DEF="-DCZ_EXPERIMENT_MX12 -D${flags#mx12:}"; variant;;
                 mx2:*) DEF="-DCZ_EXPERIMENT_MX2 -D${flags#mx2:}"; variant;;
                 define:*) DEF="-D${flags#define:}";;
                 *) GEN="--ablate $flags";; esac
  python3 tools/gen_tower_asm.py $d $GEN > /dev/null
  ( cd $d && /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt $DEF \
      -Wno-unused-function -o $OLDPWD/tools/ab/lib_mx_$name.so $SOURCES ) &
done
wait
ls -la tools/ab/
