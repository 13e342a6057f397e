# The translation units of the kernel library, their compile flags and their staleness rule.  Sourced (not run) by
# csrc/build.sh and scripts/ab_variant.sh, with $CSRC = this directory: a library either of them links holds the same units.
SRCS="gemm gemm256 gemm256_tn fp8 gemm_rows gemm_wgrad_rows conv conv_lane bnact bnfold bert attn head retrieval augment optim optim_sgd util stem"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=fast -Wno-unused-result"
unit_headers() {      # $1 = unit: the headers its object depends on
  case $1 in
    gemm|gemm256|gemm256_tn) echo "$CSRC/common_hip.h $CSRC/../../include/mammoclip_hip.h $CSRC/gemm_tile.h" ;;
    optim|optim_sgd) echo "$CSRC/common_hip.h $CSRC/../../include/mammoclip_hip.h $CSRC/multi_tensor.h" ;;
    *) echo "$CSRC/common_hip.h $CSRC/../../include/mammoclip_hip.h" ;;
  esac
}
unit_stale() {        # $1 = object directory, $2 = unit: true when the object is missing or older than its source / headers
  [ -f $1/$2.o ] || return 0
  local d
  for d in $CSRC/$2.hip $(unit_headers $2); do
    if [ $d -nt $1/$2.o ]; then return 0; fi
  done
  return 1
}
