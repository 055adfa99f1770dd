# Lab builds of the library with a SEQ_EXP timing switch in k_block_x6<.., SEQ> (results are then WRONG): tools/seqlab_<n>.so.
# usage: bash tools/seq_lab.sh 1 2 3 ...   (run where the library was built; the .so files travel with the tree)
# names: <n> = SEQ_EXP=<n>; stamp / stamp1 = phase stamps (/ per-step stamps too); builtin_dma; front0 = the front's steps in the
# order q, k, v with the three epilogues behind the v step (SEQ_FRONT_RIDE=0; the shipped form is k, v, q with riding epilogues);
# stamp_front0 = both; last0 = the model's last layer as an extra trip of the layer loop for every token, its consumed rows gathered
# from the attention tiles (SEQ_LAST_ABSORB=0; the shipped form ends the launch behind the last full layer and attends from x');
# stamp_last0 = phase stamps of that form; plan_stamp = stamps of k_plan_seq (PLAN_STAMP, tools/plan_stamps.py); io0 = the prologue
# gather and the x' stores of LayerNorm 3 as plain loads and stores, one memory round trip at a time (SEQ_BATCHED_IO=0; the shipped form
# requests the gather's 32 pieces at once and stores x' from inline asm with no wait in between); stamp_io0 = phase stamps of that form
set -e
cd "$(dirname "$0")/.."
OBJ=influentialrs_amd/csrc/_obj
for n in "$@"; do
  if [ "$n" = stamp ]; then DEF="-DX6_STAMP=2"; elif [ "$n" = stamp_builtin_dma ]; then DEF="-DX6_STAMP=2 -DSEQ_ASM_DMA=0"; elif [ "$n" = stamp1 ]; then DEF="-DX6_STAMP=1"; elif [ "$n" = builtin_dma ]; then DEF="-DSEQ_ASM_DMA=0"; elif [ "$n" = front0 ]; then DEF="-DSEQ_FRONT_RIDE=0"; elif [ "$n" = stamp_front0 ]; then DEF="-DX6_STAMP=2 -DSEQ_FRONT_RIDE=0"; elif [ "$n" = last0 ]; then DEF="-DSEQ_LAST_ABSORB=0"; elif [ "$n" = stamp_last0 ]; then DEF="-DX6_STAMP=2 -DSEQ_LAST_ABSORB=0"; elif [ "$n" = plan_stamp ]; then DEF="-DPLAN_STAMP"; elif [ "$n" = io0 ]; then DEF="-DSEQ_BATCHED_IO=0"; elif [ "$n" = stamp_io0 ]; then DEF="-DX6_STAMP=2 -DSEQ_BATCHED_IO=0"; else DEF="-DSEQ_EXP=$n"; fi
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -DIRS_LAB $DEF -c influentialrs_amd/csrc/decoder.hip -o /tmp/decoder_seqlab_$n.o 2>/dev/null
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/seqlab_$n.so $OBJ/capi.o /tmp/decoder_seqlab_$n.o $OBJ/score.o $OBJ/path.o $OBJ/comm.o $OBJ/train.o $OBJ/ce_backward.o $OBJ/ce_sharded.o $OBJ/survivors.o -ldl
  echo built tools/seqlab_$n.so
done
