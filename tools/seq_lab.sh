# Lab builds of the library with a measurement hook in decoder.hip turned on: tools/seqlab_<name>.so.
# usage: bash tools/seq_lab.sh 1 2 3 stamp ...   (run where the library was built; the .so files travel with the tree)
# names: <n> = SEQ_EXP=<n>, a timing switch in k_block_x6<.., SEQ> (results are then WRONG); stamp / stamp1 = phase stamps
# (/ per-step stamps too) of k_block_x6 (X6_STAMP, tools/seq_stamps.py); plan_stamp = stamps of k_plan_seq (PLAN_STAMP,
# tools/plan_stamps.py).  The objects beside decoder.o are the product build's: the list is influentialrs_amd/build.py's SOURCES.
set -e
cd "$(dirname "$0")/.."
OBJ=influentialrs_amd/csrc/_obj
OBJS=$(python -c "from influentialrs_amd.build import SOURCES; print(' '.join('$OBJ/' + s.replace('.hip', '.o') for s in SOURCES if s != 'decoder.hip'))")
for n in "$@"; do
  case "$n" in
    stamp) DEF="-DX6_STAMP=2" ;;
    stamp1) DEF="-DX6_STAMP=1" ;;
    plan_stamp) DEF="-DPLAN_STAMP" ;;
    [0-9]*) DEF="-DSEQ_EXP=$n" ;;
    *) echo "unknown build name: $n" >&2; exit 1 ;;
  esac
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -DIRS_LAB $DEF -c influentialrs_amd/csrc/decoder.hip -o /tmp/decoder_seqlab_$n.o 2>/dev/null
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/seqlab_$n.so /tmp/decoder_seqlab_$n.o $OBJS -ldl
  echo built tools/seqlab_$n.so
done
