"""The launch plan of k_constraint_jacobian without a GPU: plan_launch() of csrc/qln_launch_plan.h is host-only integer
arithmetic, so a small stand-alone program (tests/launch_plan_print.cpp, built with hipcc --offload-host-only) prints the plan of
every request below and the output is compared with tables written out here.

The tables were derived by reading the launch code this header replaced (launch_constraint_jacobian, launch_cj_t,
launch_c_only_t, launch_eval_all, launch_objective_and_constraint, nnz_lds_bytes and prefetch_flags of qln_kernels.hip), not
by running plan_launch(): the old launchers were transcribed line by line into a script of plain integer arithmetic, kept
outside the repository, whose output is pasted below; about twenty lines (the LDS sizes, both sides of each streaming
threshold, the prefetch and pad cases, several QLN_VARIANT ids) were recomputed by hand from the old code.  A line reads

    format outputs N nb lat [kt] [var] [env] | <T,KC,W,WITH_C,WITH_J,NNZ,SPLIT,STREAM,WITH_F> wg lds ahead what

format D / S = dense blocks / structural; outputs c, J, cJ, all (qln_eval_all) or fc (f + c); lat = the caller prefers
latency (kLaunchSplit); kt = the batch's largest k_trans (14 unless given); var = QLN_VARIANT; env = QLN_PREFETCH_AHEAD,
QLN_PREFETCH_MASK, QLN_PAD_LDS of the knob builds (-1 = unset).  wg = workgroups before xcd_grid, lds = dynamic LDS bytes, ahead =
prefetch distance in problems, what = kPrefetchNoZ | kPrefetchBnd | kPrefetchDesc shifted down to bits 0..2.

PRODUCT covers N on both sides of every boundary (17 | 18 the split, 41 | 42, 65 | 66 and 81 | 82 the chunk rule, 65 | 66 the
dense prefetch), nb in {1, 256, 257} with and without the latency preference, both formats and every output set; then each
byte formula of the 512 MiB streaming threshold on both sides (dense N = 40: 93 600 B per problem, nb = 5735 cacheable,
5736 streamed), and the dynamic LDS of the structural format at N = 40 for kt_max in {2, 14, 41}.  TUNING is the second build
(-DQLN_TUNING): every QLN_VARIANT id on both formats and every output set (an id that does not apply falls through to the
product's plan), and the environment knobs."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PRODUCT = """
D c   N=2   nb=1     lat=0 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D c   N=2   nb=1     lat=1 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D c   N=2   nb=256   lat=0 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D c   N=2   nb=256   lat=1 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D c   N=2   nb=257   lat=0 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=2   nb=257   lat=1 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=17  nb=1     lat=0 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D c   N=17  nb=1     lat=1 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D c   N=17  nb=256   lat=0 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D c   N=17  nb=256   lat=1 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D c   N=17  nb=257   lat=0 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=17  nb=257   lat=1 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=18  nb=1     lat=0 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D c   N=18  nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=2 lds=0 ahead=0 what=0
D c   N=18  nb=256   lat=0 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D c   N=18  nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=512 lds=0 ahead=0 what=0
D c   N=18  nb=257   lat=0 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=18  nb=257   lat=1 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=41  nb=1     lat=0 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D c   N=41  nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=3 lds=0 ahead=0 what=0
D c   N=41  nb=256   lat=0 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D c   N=41  nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=768 lds=0 ahead=0 what=0
D c   N=41  nb=257   lat=0 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=41  nb=257   lat=1 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=42  nb=1     lat=0 | <8,64,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D c   N=42  nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=3 lds=0 ahead=0 what=0
D c   N=42  nb=256   lat=0 | <8,64,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D c   N=42  nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=768 lds=0 ahead=0 what=0
D c   N=42  nb=257   lat=0 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=42  nb=257   lat=1 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=65  nb=1     lat=0 | <8,64,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D c   N=65  nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=4 lds=0 ahead=0 what=0
D c   N=65  nb=256   lat=0 | <8,64,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D c   N=65  nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=1024 lds=0 ahead=0 what=0
D c   N=65  nb=257   lat=0 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=65  nb=257   lat=1 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=66  nb=1     lat=0 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D c   N=66  nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=5 lds=0 ahead=0 what=0
D c   N=66  nb=256   lat=0 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D c   N=66  nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=1280 lds=0 ahead=0 what=0
D c   N=66  nb=257   lat=0 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=66  nb=257   lat=1 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=81  nb=1     lat=0 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D c   N=81  nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=5 lds=0 ahead=0 what=0
D c   N=81  nb=256   lat=0 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D c   N=81  nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=1280 lds=0 ahead=0 what=0
D c   N=81  nb=257   lat=0 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=81  nb=257   lat=1 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=82  nb=1     lat=0 | <8,64,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D c   N=82  nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=6 lds=0 ahead=0 what=0
D c   N=82  nb=256   lat=0 | <8,64,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D c   N=82  nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=1536 lds=0 ahead=0 what=0
D c   N=82  nb=257   lat=0 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=82  nb=257   lat=1 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=130 nb=1     lat=0 | <8,64,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D c   N=130 nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=9 lds=0 ahead=0 what=0
D c   N=130 nb=256   lat=0 | <8,64,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D c   N=130 nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=2304 lds=0 ahead=0 what=0
D c   N=130 nb=257   lat=0 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D c   N=130 nb=257   lat=1 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=2   nb=1     lat=0 | <12,64,1,0,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D J   N=2   nb=1     lat=1 | <12,64,1,0,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D J   N=2   nb=256   lat=0 | <12,64,1,0,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D J   N=2   nb=256   lat=1 | <12,64,1,0,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D J   N=2   nb=257   lat=0 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=2   nb=257   lat=1 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=17  nb=1     lat=0 | <12,64,1,0,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D J   N=17  nb=1     lat=1 | <12,64,1,0,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D J   N=17  nb=256   lat=0 | <12,64,1,0,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D J   N=17  nb=256   lat=1 | <12,64,1,0,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D J   N=17  nb=257   lat=0 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=17  nb=257   lat=1 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=18  nb=1     lat=0 | <12,64,1,0,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D J   N=18  nb=1     lat=1 | <16,16,1,0,1,0,1,0,0> wg=2 lds=0 ahead=0 what=0
D J   N=18  nb=256   lat=0 | <12,64,1,0,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D J   N=18  nb=256   lat=1 | <16,16,1,0,1,0,1,0,0> wg=512 lds=0 ahead=0 what=0
D J   N=18  nb=257   lat=0 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=18  nb=257   lat=1 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=41  nb=1     lat=0 | <12,64,1,0,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D J   N=41  nb=1     lat=1 | <16,16,1,0,1,0,1,0,0> wg=3 lds=0 ahead=0 what=0
D J   N=41  nb=256   lat=0 | <12,64,1,0,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D J   N=41  nb=256   lat=1 | <16,16,1,0,1,0,1,0,0> wg=768 lds=0 ahead=0 what=0
D J   N=41  nb=257   lat=0 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=41  nb=257   lat=1 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=42  nb=1     lat=0 | <12,64,1,0,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D J   N=42  nb=1     lat=1 | <16,16,1,0,1,0,1,0,0> wg=3 lds=0 ahead=0 what=0
D J   N=42  nb=256   lat=0 | <12,64,1,0,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D J   N=42  nb=256   lat=1 | <16,16,1,0,1,0,1,0,0> wg=768 lds=0 ahead=0 what=0
D J   N=42  nb=257   lat=0 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=42  nb=257   lat=1 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=65  nb=1     lat=0 | <12,64,1,0,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D J   N=65  nb=1     lat=1 | <16,16,1,0,1,0,1,0,0> wg=4 lds=0 ahead=0 what=0
D J   N=65  nb=256   lat=0 | <12,64,1,0,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D J   N=65  nb=256   lat=1 | <16,16,1,0,1,0,1,0,0> wg=1024 lds=0 ahead=0 what=0
D J   N=65  nb=257   lat=0 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=65  nb=257   lat=1 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=66  nb=1     lat=0 | <12,64,1,0,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D J   N=66  nb=1     lat=1 | <16,16,1,0,1,0,1,0,0> wg=5 lds=0 ahead=0 what=0
D J   N=66  nb=256   lat=0 | <12,64,1,0,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D J   N=66  nb=256   lat=1 | <16,16,1,0,1,0,1,0,0> wg=1280 lds=0 ahead=0 what=0
D J   N=66  nb=257   lat=0 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=66  nb=257   lat=1 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=81  nb=1     lat=0 | <12,64,1,0,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D J   N=81  nb=1     lat=1 | <16,16,1,0,1,0,1,0,0> wg=5 lds=0 ahead=0 what=0
D J   N=81  nb=256   lat=0 | <12,64,1,0,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D J   N=81  nb=256   lat=1 | <16,16,1,0,1,0,1,0,0> wg=1280 lds=0 ahead=0 what=0
D J   N=81  nb=257   lat=0 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=81  nb=257   lat=1 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=82  nb=1     lat=0 | <12,64,1,0,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D J   N=82  nb=1     lat=1 | <16,16,1,0,1,0,1,0,0> wg=6 lds=0 ahead=0 what=0
D J   N=82  nb=256   lat=0 | <12,64,1,0,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D J   N=82  nb=256   lat=1 | <16,16,1,0,1,0,1,0,0> wg=1536 lds=0 ahead=0 what=0
D J   N=82  nb=257   lat=0 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=82  nb=257   lat=1 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=130 nb=1     lat=0 | <12,64,1,0,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D J   N=130 nb=1     lat=1 | <16,16,1,0,1,0,1,0,0> wg=9 lds=0 ahead=0 what=0
D J   N=130 nb=256   lat=0 | <12,64,1,0,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D J   N=130 nb=256   lat=1 | <16,16,1,0,1,0,1,0,0> wg=2304 lds=0 ahead=0 what=0
D J   N=130 nb=257   lat=0 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D J   N=130 nb=257   lat=1 | <12,64,1,0,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D cJ  N=2   nb=1     lat=0 | <12,64,1,1,1,0,0,0,0> wg=1 lds=0 ahead=64 what=0
D cJ  N=2   nb=1     lat=1 | <12,64,1,1,1,0,0,0,0> wg=1 lds=0 ahead=64 what=0
D cJ  N=2   nb=256   lat=0 | <12,64,1,1,1,0,0,0,0> wg=256 lds=0 ahead=64 what=0
D cJ  N=2   nb=256   lat=1 | <12,64,1,1,1,0,0,0,0> wg=256 lds=0 ahead=64 what=0
D cJ  N=2   nb=257   lat=0 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=64 what=0
D cJ  N=2   nb=257   lat=1 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=64 what=0
D cJ  N=17  nb=1     lat=0 | <12,64,1,1,1,0,0,0,0> wg=1 lds=0 ahead=64 what=0
D cJ  N=17  nb=1     lat=1 | <12,64,1,1,1,0,0,0,0> wg=1 lds=0 ahead=64 what=0
D cJ  N=17  nb=256   lat=0 | <12,64,1,1,1,0,0,0,0> wg=256 lds=0 ahead=64 what=0
D cJ  N=17  nb=256   lat=1 | <12,64,1,1,1,0,0,0,0> wg=256 lds=0 ahead=64 what=0
D cJ  N=17  nb=257   lat=0 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=64 what=0
D cJ  N=17  nb=257   lat=1 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=64 what=0
D cJ  N=18  nb=1     lat=0 | <12,64,1,1,1,0,0,0,0> wg=1 lds=0 ahead=64 what=0
D cJ  N=18  nb=1     lat=1 | <16,16,1,1,1,0,1,0,0> wg=2 lds=0 ahead=0 what=0
D cJ  N=18  nb=256   lat=0 | <12,64,1,1,1,0,0,0,0> wg=256 lds=0 ahead=64 what=0
D cJ  N=18  nb=256   lat=1 | <16,16,1,1,1,0,1,0,0> wg=512 lds=0 ahead=0 what=0
D cJ  N=18  nb=257   lat=0 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=64 what=0
D cJ  N=18  nb=257   lat=1 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=64 what=0
D cJ  N=41  nb=1     lat=0 | <12,64,1,1,1,0,0,0,0> wg=1 lds=0 ahead=64 what=0
D cJ  N=41  nb=1     lat=1 | <16,16,1,1,1,0,1,0,0> wg=3 lds=0 ahead=0 what=0
D cJ  N=41  nb=256   lat=0 | <12,64,1,1,1,0,0,0,0> wg=256 lds=0 ahead=64 what=0
D cJ  N=41  nb=256   lat=1 | <16,16,1,1,1,0,1,0,0> wg=768 lds=0 ahead=0 what=0
D cJ  N=41  nb=257   lat=0 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=64 what=0
D cJ  N=41  nb=257   lat=1 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=64 what=0
D cJ  N=42  nb=1     lat=0 | <12,64,1,1,1,0,0,0,0> wg=1 lds=0 ahead=64 what=0
D cJ  N=42  nb=1     lat=1 | <16,16,1,1,1,0,1,0,0> wg=3 lds=0 ahead=0 what=0
D cJ  N=42  nb=256   lat=0 | <12,64,1,1,1,0,0,0,0> wg=256 lds=0 ahead=64 what=0
D cJ  N=42  nb=256   lat=1 | <16,16,1,1,1,0,1,0,0> wg=768 lds=0 ahead=0 what=0
D cJ  N=42  nb=257   lat=0 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=64 what=0
D cJ  N=42  nb=257   lat=1 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=64 what=0
D cJ  N=65  nb=1     lat=0 | <12,64,1,1,1,0,0,0,0> wg=1 lds=0 ahead=64 what=0
D cJ  N=65  nb=1     lat=1 | <16,16,1,1,1,0,1,0,0> wg=4 lds=0 ahead=0 what=0
D cJ  N=65  nb=256   lat=0 | <12,64,1,1,1,0,0,0,0> wg=256 lds=0 ahead=64 what=0
D cJ  N=65  nb=256   lat=1 | <16,16,1,1,1,0,1,0,0> wg=1024 lds=0 ahead=0 what=0
D cJ  N=65  nb=257   lat=0 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=64 what=0
D cJ  N=65  nb=257   lat=1 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=64 what=0
D cJ  N=66  nb=1     lat=0 | <12,64,1,1,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D cJ  N=66  nb=1     lat=1 | <16,16,1,1,1,0,1,0,0> wg=5 lds=0 ahead=0 what=0
D cJ  N=66  nb=256   lat=0 | <12,64,1,1,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D cJ  N=66  nb=256   lat=1 | <16,16,1,1,1,0,1,0,0> wg=1280 lds=0 ahead=0 what=0
D cJ  N=66  nb=257   lat=0 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D cJ  N=66  nb=257   lat=1 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D cJ  N=81  nb=1     lat=0 | <12,64,1,1,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D cJ  N=81  nb=1     lat=1 | <16,16,1,1,1,0,1,0,0> wg=5 lds=0 ahead=0 what=0
D cJ  N=81  nb=256   lat=0 | <12,64,1,1,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D cJ  N=81  nb=256   lat=1 | <16,16,1,1,1,0,1,0,0> wg=1280 lds=0 ahead=0 what=0
D cJ  N=81  nb=257   lat=0 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D cJ  N=81  nb=257   lat=1 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D cJ  N=82  nb=1     lat=0 | <12,64,1,1,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D cJ  N=82  nb=1     lat=1 | <16,16,1,1,1,0,1,0,0> wg=6 lds=0 ahead=0 what=0
D cJ  N=82  nb=256   lat=0 | <12,64,1,1,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D cJ  N=82  nb=256   lat=1 | <16,16,1,1,1,0,1,0,0> wg=1536 lds=0 ahead=0 what=0
D cJ  N=82  nb=257   lat=0 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D cJ  N=82  nb=257   lat=1 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D cJ  N=130 nb=1     lat=0 | <12,64,1,1,1,0,0,0,0> wg=1 lds=0 ahead=0 what=0
D cJ  N=130 nb=1     lat=1 | <16,16,1,1,1,0,1,0,0> wg=9 lds=0 ahead=0 what=0
D cJ  N=130 nb=256   lat=0 | <12,64,1,1,1,0,0,0,0> wg=256 lds=0 ahead=0 what=0
D cJ  N=130 nb=256   lat=1 | <16,16,1,1,1,0,1,0,0> wg=2304 lds=0 ahead=0 what=0
D cJ  N=130 nb=257   lat=0 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D cJ  N=130 nb=257   lat=1 | <12,64,1,1,1,0,0,0,0> wg=257 lds=0 ahead=0 what=0
D all N=2   nb=1     lat=0 | <16,64,1,1,1,0,0,0,1> wg=1 lds=0 ahead=64 what=6
D all N=2   nb=256   lat=0 | <16,64,1,1,1,0,0,0,1> wg=256 lds=0 ahead=64 what=6
D all N=2   nb=257   lat=0 | <16,64,1,1,1,0,0,0,1> wg=257 lds=0 ahead=64 what=6
D all N=17  nb=1     lat=0 | <16,64,1,1,1,0,0,0,1> wg=1 lds=0 ahead=64 what=6
D all N=17  nb=256   lat=0 | <16,64,1,1,1,0,0,0,1> wg=256 lds=0 ahead=64 what=6
D all N=17  nb=257   lat=0 | <16,64,1,1,1,0,0,0,1> wg=257 lds=0 ahead=64 what=6
D all N=18  nb=1     lat=0 | <16,64,1,1,1,0,0,0,1> wg=1 lds=0 ahead=64 what=6
D all N=18  nb=256   lat=0 | <16,64,1,1,1,0,0,0,1> wg=256 lds=0 ahead=64 what=6
D all N=18  nb=257   lat=0 | <16,64,1,1,1,0,0,0,1> wg=257 lds=0 ahead=64 what=6
D all N=41  nb=1     lat=0 | <16,64,1,1,1,0,0,0,1> wg=1 lds=0 ahead=64 what=6
D all N=41  nb=256   lat=0 | <16,64,1,1,1,0,0,0,1> wg=256 lds=0 ahead=64 what=6
D all N=41  nb=257   lat=0 | <16,64,1,1,1,0,0,0,1> wg=257 lds=0 ahead=64 what=6
D all N=42  nb=1     lat=0 | <16,64,1,1,1,0,0,0,1> wg=1 lds=0 ahead=64 what=6
D all N=42  nb=256   lat=0 | <16,64,1,1,1,0,0,0,1> wg=256 lds=0 ahead=64 what=6
D all N=42  nb=257   lat=0 | <16,64,1,1,1,0,0,0,1> wg=257 lds=0 ahead=64 what=6
D all N=65  nb=1     lat=0 | <16,64,1,1,1,0,0,0,1> wg=1 lds=0 ahead=64 what=6
D all N=65  nb=256   lat=0 | <16,64,1,1,1,0,0,0,1> wg=256 lds=0 ahead=64 what=6
D all N=65  nb=257   lat=0 | <16,64,1,1,1,0,0,0,1> wg=257 lds=0 ahead=64 what=6
D all N=66  nb=1     lat=0 | <16,64,1,1,1,0,0,0,1> wg=1 lds=0 ahead=0 what=0
D all N=66  nb=256   lat=0 | <16,64,1,1,1,0,0,0,1> wg=256 lds=0 ahead=0 what=0
D all N=66  nb=257   lat=0 | <16,64,1,1,1,0,0,0,1> wg=257 lds=0 ahead=0 what=0
D all N=81  nb=1     lat=0 | <16,64,1,1,1,0,0,0,1> wg=1 lds=0 ahead=0 what=0
D all N=81  nb=256   lat=0 | <16,64,1,1,1,0,0,0,1> wg=256 lds=0 ahead=0 what=0
D all N=81  nb=257   lat=0 | <16,64,1,1,1,0,0,0,1> wg=257 lds=0 ahead=0 what=0
D all N=82  nb=1     lat=0 | <16,64,1,1,1,0,0,0,1> wg=1 lds=0 ahead=0 what=0
D all N=82  nb=256   lat=0 | <16,64,1,1,1,0,0,0,1> wg=256 lds=0 ahead=0 what=0
D all N=82  nb=257   lat=0 | <16,64,1,1,1,0,0,0,1> wg=257 lds=0 ahead=0 what=0
D all N=130 nb=1     lat=0 | <16,64,1,1,1,0,0,0,1> wg=1 lds=0 ahead=0 what=0
D all N=130 nb=256   lat=0 | <16,64,1,1,1,0,0,0,1> wg=256 lds=0 ahead=0 what=0
D all N=130 nb=257   lat=0 | <16,64,1,1,1,0,0,0,1> wg=257 lds=0 ahead=0 what=0
D fc  N=2   nb=1     lat=0 | <5,40,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
D fc  N=2   nb=256   lat=0 | <5,40,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
D fc  N=2   nb=257   lat=0 | <5,40,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
D fc  N=17  nb=1     lat=0 | <5,40,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
D fc  N=17  nb=256   lat=0 | <5,40,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
D fc  N=17  nb=257   lat=0 | <5,40,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
D fc  N=18  nb=1     lat=0 | <5,40,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
D fc  N=18  nb=256   lat=0 | <5,40,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
D fc  N=18  nb=257   lat=0 | <5,40,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
D fc  N=41  nb=1     lat=0 | <5,40,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
D fc  N=41  nb=256   lat=0 | <5,40,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
D fc  N=41  nb=257   lat=0 | <5,40,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
D fc  N=42  nb=1     lat=0 | <8,64,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
D fc  N=42  nb=256   lat=0 | <8,64,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
D fc  N=42  nb=257   lat=0 | <8,64,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
D fc  N=65  nb=1     lat=0 | <8,64,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
D fc  N=65  nb=256   lat=0 | <8,64,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
D fc  N=65  nb=257   lat=0 | <8,64,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
D fc  N=66  nb=1     lat=0 | <5,40,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
D fc  N=66  nb=256   lat=0 | <5,40,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
D fc  N=66  nb=257   lat=0 | <5,40,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
D fc  N=81  nb=1     lat=0 | <5,40,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
D fc  N=81  nb=256   lat=0 | <5,40,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
D fc  N=81  nb=257   lat=0 | <5,40,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
D fc  N=82  nb=1     lat=0 | <8,64,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
D fc  N=82  nb=256   lat=0 | <8,64,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
D fc  N=82  nb=257   lat=0 | <8,64,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
D fc  N=130 nb=1     lat=0 | <8,64,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
D fc  N=130 nb=256   lat=0 | <8,64,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
D fc  N=130 nb=257   lat=0 | <8,64,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
S c   N=2   nb=1     lat=0 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
S c   N=2   nb=1     lat=1 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
S c   N=2   nb=256   lat=0 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
S c   N=2   nb=256   lat=1 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
S c   N=2   nb=257   lat=0 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=2   nb=257   lat=1 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=17  nb=1     lat=0 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
S c   N=17  nb=1     lat=1 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
S c   N=17  nb=256   lat=0 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
S c   N=17  nb=256   lat=1 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
S c   N=17  nb=257   lat=0 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=17  nb=257   lat=1 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=18  nb=1     lat=0 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
S c   N=18  nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=2 lds=0 ahead=0 what=0
S c   N=18  nb=256   lat=0 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
S c   N=18  nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=512 lds=0 ahead=0 what=0
S c   N=18  nb=257   lat=0 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=18  nb=257   lat=1 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=41  nb=1     lat=0 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
S c   N=41  nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=3 lds=0 ahead=0 what=0
S c   N=41  nb=256   lat=0 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
S c   N=41  nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=768 lds=0 ahead=0 what=0
S c   N=41  nb=257   lat=0 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=41  nb=257   lat=1 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=42  nb=1     lat=0 | <8,64,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
S c   N=42  nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=3 lds=0 ahead=0 what=0
S c   N=42  nb=256   lat=0 | <8,64,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
S c   N=42  nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=768 lds=0 ahead=0 what=0
S c   N=42  nb=257   lat=0 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=42  nb=257   lat=1 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=65  nb=1     lat=0 | <8,64,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
S c   N=65  nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=4 lds=0 ahead=0 what=0
S c   N=65  nb=256   lat=0 | <8,64,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
S c   N=65  nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=1024 lds=0 ahead=0 what=0
S c   N=65  nb=257   lat=0 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=65  nb=257   lat=1 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=66  nb=1     lat=0 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
S c   N=66  nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=5 lds=0 ahead=0 what=0
S c   N=66  nb=256   lat=0 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
S c   N=66  nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=1280 lds=0 ahead=0 what=0
S c   N=66  nb=257   lat=0 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=66  nb=257   lat=1 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=81  nb=1     lat=0 | <5,40,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
S c   N=81  nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=5 lds=0 ahead=0 what=0
S c   N=81  nb=256   lat=0 | <5,40,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
S c   N=81  nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=1280 lds=0 ahead=0 what=0
S c   N=81  nb=257   lat=0 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=81  nb=257   lat=1 | <5,40,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=82  nb=1     lat=0 | <8,64,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
S c   N=82  nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=6 lds=0 ahead=0 what=0
S c   N=82  nb=256   lat=0 | <8,64,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
S c   N=82  nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=1536 lds=0 ahead=0 what=0
S c   N=82  nb=257   lat=0 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=82  nb=257   lat=1 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=130 nb=1     lat=0 | <8,64,2,1,0,0,0,0,0> wg=1 lds=0 ahead=0 what=0
S c   N=130 nb=1     lat=1 | <16,16,1,1,0,0,1,0,0> wg=9 lds=0 ahead=0 what=0
S c   N=130 nb=256   lat=0 | <8,64,2,1,0,0,0,0,0> wg=256 lds=0 ahead=0 what=0
S c   N=130 nb=256   lat=1 | <16,16,1,1,0,0,1,0,0> wg=2304 lds=0 ahead=0 what=0
S c   N=130 nb=257   lat=0 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S c   N=130 nb=257   lat=1 | <8,64,2,1,0,0,0,0,0> wg=257 lds=0 ahead=0 what=0
S J   N=2   nb=1     lat=0 | <0,40,1,0,1,1,0,0,0> wg=1 lds=11328 ahead=0 what=0
S J   N=2   nb=1     lat=1 | <0,40,1,0,1,1,0,0,0> wg=1 lds=11328 ahead=0 what=0
S J   N=2   nb=256   lat=0 | <0,40,1,0,1,1,0,0,0> wg=256 lds=11328 ahead=0 what=0
S J   N=2   nb=256   lat=1 | <0,40,1,0,1,1,0,0,0> wg=256 lds=11328 ahead=0 what=0
S J   N=2   nb=257   lat=0 | <0,40,1,0,1,1,0,0,0> wg=257 lds=11328 ahead=0 what=0
S J   N=2   nb=257   lat=1 | <0,40,1,0,1,1,0,0,0> wg=257 lds=11328 ahead=0 what=0
S J   N=17  nb=1     lat=0 | <0,40,1,0,1,1,0,0,0> wg=1 lds=11328 ahead=0 what=0
S J   N=17  nb=1     lat=1 | <0,40,1,0,1,1,0,0,0> wg=1 lds=11328 ahead=0 what=0
S J   N=17  nb=256   lat=0 | <0,40,1,0,1,1,0,0,0> wg=256 lds=11328 ahead=0 what=0
S J   N=17  nb=256   lat=1 | <0,40,1,0,1,1,0,0,0> wg=256 lds=11328 ahead=0 what=0
S J   N=17  nb=257   lat=0 | <0,40,1,0,1,1,0,0,0> wg=257 lds=11328 ahead=0 what=0
S J   N=17  nb=257   lat=1 | <0,40,1,0,1,1,0,0,0> wg=257 lds=11328 ahead=0 what=0
S J   N=18  nb=1     lat=0 | <0,40,1,0,1,1,0,0,0> wg=1 lds=11328 ahead=0 what=0
S J   N=18  nb=1     lat=1 | <0,16,2,0,1,1,1,0,0> wg=2 lds=8656 ahead=0 what=0
S J   N=18  nb=256   lat=0 | <0,40,1,0,1,1,0,0,0> wg=256 lds=11328 ahead=0 what=0
S J   N=18  nb=256   lat=1 | <0,16,2,0,1,1,1,0,0> wg=512 lds=8656 ahead=0 what=0
S J   N=18  nb=257   lat=0 | <0,40,1,0,1,1,0,0,0> wg=257 lds=11328 ahead=0 what=0
S J   N=18  nb=257   lat=1 | <0,40,1,0,1,1,0,0,0> wg=257 lds=11328 ahead=0 what=0
S J   N=41  nb=1     lat=0 | <0,40,1,0,1,1,0,0,0> wg=1 lds=19600 ahead=0 what=0
S J   N=41  nb=1     lat=1 | <0,16,2,0,1,1,1,0,0> wg=3 lds=8656 ahead=0 what=0
S J   N=41  nb=256   lat=0 | <0,40,1,0,1,1,0,0,0> wg=256 lds=19600 ahead=0 what=0
S J   N=41  nb=256   lat=1 | <0,16,2,0,1,1,1,0,0> wg=768 lds=8656 ahead=0 what=0
S J   N=41  nb=257   lat=0 | <0,40,1,0,1,1,0,0,0> wg=257 lds=19600 ahead=0 what=0
S J   N=41  nb=257   lat=1 | <0,40,1,0,1,1,0,0,0> wg=257 lds=19600 ahead=0 what=0
S J   N=42  nb=1     lat=0 | <0,64,1,0,1,1,0,0,0> wg=1 lds=20064 ahead=0 what=0
S J   N=42  nb=1     lat=1 | <0,16,2,0,1,1,1,0,0> wg=3 lds=8656 ahead=0 what=0
S J   N=42  nb=256   lat=0 | <0,64,1,0,1,1,0,0,0> wg=256 lds=20064 ahead=0 what=0
S J   N=42  nb=256   lat=1 | <0,16,2,0,1,1,1,0,0> wg=768 lds=8656 ahead=0 what=0
S J   N=42  nb=257   lat=0 | <0,64,1,0,1,1,0,0,0> wg=257 lds=20064 ahead=0 what=0
S J   N=42  nb=257   lat=1 | <0,64,1,0,1,1,0,0,0> wg=257 lds=20064 ahead=0 what=0
S J   N=65  nb=1     lat=0 | <0,64,1,0,1,1,0,0,0> wg=1 lds=30544 ahead=0 what=0
S J   N=65  nb=1     lat=1 | <0,16,2,0,1,1,1,0,0> wg=4 lds=8656 ahead=0 what=0
S J   N=65  nb=256   lat=0 | <0,64,1,0,1,1,0,0,0> wg=256 lds=30544 ahead=0 what=0
S J   N=65  nb=256   lat=1 | <0,16,2,0,1,1,1,0,0> wg=1024 lds=8656 ahead=0 what=0
S J   N=65  nb=257   lat=0 | <0,64,1,0,1,1,0,0,0> wg=257 lds=30544 ahead=0 what=0
S J   N=65  nb=257   lat=1 | <0,64,1,0,1,1,0,0,0> wg=257 lds=30544 ahead=0 what=0
S J   N=66  nb=1     lat=0 | <0,40,1,0,1,1,0,0,0> wg=1 lds=19600 ahead=0 what=0
S J   N=66  nb=1     lat=1 | <0,16,2,0,1,1,1,0,0> wg=5 lds=8656 ahead=0 what=0
S J   N=66  nb=256   lat=0 | <0,40,1,0,1,1,0,0,0> wg=256 lds=19600 ahead=0 what=0
S J   N=66  nb=256   lat=1 | <0,16,2,0,1,1,1,0,0> wg=1280 lds=8656 ahead=0 what=0
S J   N=66  nb=257   lat=0 | <0,40,1,0,1,1,0,0,0> wg=257 lds=19600 ahead=0 what=0
S J   N=66  nb=257   lat=1 | <0,40,1,0,1,1,0,0,0> wg=257 lds=19600 ahead=0 what=0
S J   N=81  nb=1     lat=0 | <0,40,1,0,1,1,0,0,0> wg=1 lds=19600 ahead=0 what=0
S J   N=81  nb=1     lat=1 | <0,16,2,0,1,1,1,0,0> wg=5 lds=8656 ahead=0 what=0
S J   N=81  nb=256   lat=0 | <0,40,1,0,1,1,0,0,0> wg=256 lds=19600 ahead=0 what=0
S J   N=81  nb=256   lat=1 | <0,16,2,0,1,1,1,0,0> wg=1280 lds=8656 ahead=0 what=0
S J   N=81  nb=257   lat=0 | <0,40,1,0,1,1,0,0,0> wg=257 lds=19600 ahead=0 what=0
S J   N=81  nb=257   lat=1 | <0,40,1,0,1,1,0,0,0> wg=257 lds=19600 ahead=0 what=0
S J   N=82  nb=1     lat=0 | <0,64,1,0,1,1,0,0,0> wg=1 lds=30544 ahead=0 what=0
S J   N=82  nb=1     lat=1 | <0,16,2,0,1,1,1,0,0> wg=6 lds=8656 ahead=0 what=0
S J   N=82  nb=256   lat=0 | <0,64,1,0,1,1,0,0,0> wg=256 lds=30544 ahead=0 what=0
S J   N=82  nb=256   lat=1 | <0,16,2,0,1,1,1,0,0> wg=1536 lds=8656 ahead=0 what=0
S J   N=82  nb=257   lat=0 | <0,64,1,0,1,1,0,0,0> wg=257 lds=30544 ahead=0 what=0
S J   N=82  nb=257   lat=1 | <0,64,1,0,1,1,0,0,0> wg=257 lds=30544 ahead=0 what=0
S J   N=130 nb=1     lat=0 | <0,64,1,0,1,1,0,0,0> wg=1 lds=30544 ahead=0 what=0
S J   N=130 nb=1     lat=1 | <0,16,2,0,1,1,1,0,0> wg=9 lds=8656 ahead=0 what=0
S J   N=130 nb=256   lat=0 | <0,64,1,0,1,1,0,0,0> wg=256 lds=30544 ahead=0 what=0
S J   N=130 nb=256   lat=1 | <0,16,2,0,1,1,1,0,0> wg=2304 lds=8656 ahead=0 what=0
S J   N=130 nb=257   lat=0 | <0,64,1,0,1,1,0,0,0> wg=257 lds=30544 ahead=0 what=0
S J   N=130 nb=257   lat=1 | <0,64,1,0,1,1,0,0,0> wg=257 lds=30544 ahead=0 what=0
S cJ  N=2   nb=1     lat=0 | <0,40,1,1,1,1,0,0,0> wg=1 lds=11328 ahead=0 what=0
S cJ  N=2   nb=1     lat=1 | <0,40,1,1,1,1,0,0,0> wg=1 lds=11328 ahead=0 what=0
S cJ  N=2   nb=256   lat=0 | <0,40,1,1,1,1,0,0,0> wg=256 lds=11328 ahead=0 what=0
S cJ  N=2   nb=256   lat=1 | <0,40,1,1,1,1,0,0,0> wg=256 lds=11328 ahead=0 what=0
S cJ  N=2   nb=257   lat=0 | <0,40,1,1,1,1,0,0,0> wg=257 lds=11328 ahead=0 what=0
S cJ  N=2   nb=257   lat=1 | <0,40,1,1,1,1,0,0,0> wg=257 lds=11328 ahead=0 what=0
S cJ  N=17  nb=1     lat=0 | <0,40,1,1,1,1,0,0,0> wg=1 lds=11328 ahead=0 what=0
S cJ  N=17  nb=1     lat=1 | <0,40,1,1,1,1,0,0,0> wg=1 lds=11328 ahead=0 what=0
S cJ  N=17  nb=256   lat=0 | <0,40,1,1,1,1,0,0,0> wg=256 lds=11328 ahead=0 what=0
S cJ  N=17  nb=256   lat=1 | <0,40,1,1,1,1,0,0,0> wg=256 lds=11328 ahead=0 what=0
S cJ  N=17  nb=257   lat=0 | <0,40,1,1,1,1,0,0,0> wg=257 lds=11328 ahead=0 what=0
S cJ  N=17  nb=257   lat=1 | <0,40,1,1,1,1,0,0,0> wg=257 lds=11328 ahead=0 what=0
S cJ  N=18  nb=1     lat=0 | <0,40,1,1,1,1,0,0,0> wg=1 lds=11328 ahead=0 what=0
S cJ  N=18  nb=1     lat=1 | <0,16,2,1,1,1,1,0,0> wg=2 lds=8656 ahead=0 what=0
S cJ  N=18  nb=256   lat=0 | <0,40,1,1,1,1,0,0,0> wg=256 lds=11328 ahead=0 what=0
S cJ  N=18  nb=256   lat=1 | <0,16,2,1,1,1,1,0,0> wg=512 lds=8656 ahead=0 what=0
S cJ  N=18  nb=257   lat=0 | <0,40,1,1,1,1,0,0,0> wg=257 lds=11328 ahead=0 what=0
S cJ  N=18  nb=257   lat=1 | <0,40,1,1,1,1,0,0,0> wg=257 lds=11328 ahead=0 what=0
S cJ  N=41  nb=1     lat=0 | <0,40,1,1,1,1,0,0,0> wg=1 lds=19600 ahead=0 what=0
S cJ  N=41  nb=1     lat=1 | <0,16,2,1,1,1,1,0,0> wg=3 lds=8656 ahead=0 what=0
S cJ  N=41  nb=256   lat=0 | <0,40,1,1,1,1,0,0,0> wg=256 lds=19600 ahead=0 what=0
S cJ  N=41  nb=256   lat=1 | <0,16,2,1,1,1,1,0,0> wg=768 lds=8656 ahead=0 what=0
S cJ  N=41  nb=257   lat=0 | <0,40,1,1,1,1,0,0,0> wg=257 lds=19600 ahead=0 what=0
S cJ  N=41  nb=257   lat=1 | <0,40,1,1,1,1,0,0,0> wg=257 lds=19600 ahead=0 what=0
S cJ  N=42  nb=1     lat=0 | <0,64,1,1,1,1,0,0,0> wg=1 lds=20064 ahead=0 what=0
S cJ  N=42  nb=1     lat=1 | <0,16,2,1,1,1,1,0,0> wg=3 lds=8656 ahead=0 what=0
S cJ  N=42  nb=256   lat=0 | <0,64,1,1,1,1,0,0,0> wg=256 lds=20064 ahead=0 what=0
S cJ  N=42  nb=256   lat=1 | <0,16,2,1,1,1,1,0,0> wg=768 lds=8656 ahead=0 what=0
S cJ  N=42  nb=257   lat=0 | <0,64,1,1,1,1,0,0,0> wg=257 lds=20064 ahead=0 what=0
S cJ  N=42  nb=257   lat=1 | <0,64,1,1,1,1,0,0,0> wg=257 lds=20064 ahead=0 what=0
S cJ  N=65  nb=1     lat=0 | <0,64,1,1,1,1,0,0,0> wg=1 lds=30544 ahead=0 what=0
S cJ  N=65  nb=1     lat=1 | <0,16,2,1,1,1,1,0,0> wg=4 lds=8656 ahead=0 what=0
S cJ  N=65  nb=256   lat=0 | <0,64,1,1,1,1,0,0,0> wg=256 lds=30544 ahead=0 what=0
S cJ  N=65  nb=256   lat=1 | <0,16,2,1,1,1,1,0,0> wg=1024 lds=8656 ahead=0 what=0
S cJ  N=65  nb=257   lat=0 | <0,64,1,1,1,1,0,0,0> wg=257 lds=30544 ahead=0 what=0
S cJ  N=65  nb=257   lat=1 | <0,64,1,1,1,1,0,0,0> wg=257 lds=30544 ahead=0 what=0
S cJ  N=66  nb=1     lat=0 | <0,40,1,1,1,1,0,0,0> wg=1 lds=19600 ahead=0 what=0
S cJ  N=66  nb=1     lat=1 | <0,16,2,1,1,1,1,0,0> wg=5 lds=8656 ahead=0 what=0
S cJ  N=66  nb=256   lat=0 | <0,40,1,1,1,1,0,0,0> wg=256 lds=19600 ahead=0 what=0
S cJ  N=66  nb=256   lat=1 | <0,16,2,1,1,1,1,0,0> wg=1280 lds=8656 ahead=0 what=0
S cJ  N=66  nb=257   lat=0 | <0,40,1,1,1,1,0,0,0> wg=257 lds=19600 ahead=0 what=0
S cJ  N=66  nb=257   lat=1 | <0,40,1,1,1,1,0,0,0> wg=257 lds=19600 ahead=0 what=0
S cJ  N=81  nb=1     lat=0 | <0,40,1,1,1,1,0,0,0> wg=1 lds=19600 ahead=0 what=0
S cJ  N=81  nb=1     lat=1 | <0,16,2,1,1,1,1,0,0> wg=5 lds=8656 ahead=0 what=0
S cJ  N=81  nb=256   lat=0 | <0,40,1,1,1,1,0,0,0> wg=256 lds=19600 ahead=0 what=0
S cJ  N=81  nb=256   lat=1 | <0,16,2,1,1,1,1,0,0> wg=1280 lds=8656 ahead=0 what=0
S cJ  N=81  nb=257   lat=0 | <0,40,1,1,1,1,0,0,0> wg=257 lds=19600 ahead=0 what=0
S cJ  N=81  nb=257   lat=1 | <0,40,1,1,1,1,0,0,0> wg=257 lds=19600 ahead=0 what=0
S cJ  N=82  nb=1     lat=0 | <0,64,1,1,1,1,0,0,0> wg=1 lds=30544 ahead=0 what=0
S cJ  N=82  nb=1     lat=1 | <0,16,2,1,1,1,1,0,0> wg=6 lds=8656 ahead=0 what=0
S cJ  N=82  nb=256   lat=0 | <0,64,1,1,1,1,0,0,0> wg=256 lds=30544 ahead=0 what=0
S cJ  N=82  nb=256   lat=1 | <0,16,2,1,1,1,1,0,0> wg=1536 lds=8656 ahead=0 what=0
S cJ  N=82  nb=257   lat=0 | <0,64,1,1,1,1,0,0,0> wg=257 lds=30544 ahead=0 what=0
S cJ  N=82  nb=257   lat=1 | <0,64,1,1,1,1,0,0,0> wg=257 lds=30544 ahead=0 what=0
S cJ  N=130 nb=1     lat=0 | <0,64,1,1,1,1,0,0,0> wg=1 lds=30544 ahead=0 what=0
S cJ  N=130 nb=1     lat=1 | <0,16,2,1,1,1,1,0,0> wg=9 lds=8656 ahead=0 what=0
S cJ  N=130 nb=256   lat=0 | <0,64,1,1,1,1,0,0,0> wg=256 lds=30544 ahead=0 what=0
S cJ  N=130 nb=256   lat=1 | <0,16,2,1,1,1,1,0,0> wg=2304 lds=8656 ahead=0 what=0
S cJ  N=130 nb=257   lat=0 | <0,64,1,1,1,1,0,0,0> wg=257 lds=30544 ahead=0 what=0
S cJ  N=130 nb=257   lat=1 | <0,64,1,1,1,1,0,0,0> wg=257 lds=30544 ahead=0 what=0
S all N=2   nb=1     lat=0 | <0,40,1,1,1,1,0,0,1> wg=1 lds=11840 ahead=0 what=0
S all N=2   nb=256   lat=0 | <0,40,1,1,1,1,0,0,1> wg=256 lds=11840 ahead=0 what=0
S all N=2   nb=257   lat=0 | <0,40,1,1,1,1,0,0,1> wg=257 lds=11840 ahead=0 what=0
S all N=17  nb=1     lat=0 | <0,40,1,1,1,1,0,0,1> wg=1 lds=11840 ahead=0 what=0
S all N=17  nb=256   lat=0 | <0,40,1,1,1,1,0,0,1> wg=256 lds=11840 ahead=0 what=0
S all N=17  nb=257   lat=0 | <0,40,1,1,1,1,0,0,1> wg=257 lds=11840 ahead=0 what=0
S all N=18  nb=1     lat=0 | <0,40,1,1,1,1,0,0,1> wg=1 lds=11840 ahead=0 what=0
S all N=18  nb=256   lat=0 | <0,40,1,1,1,1,0,0,1> wg=256 lds=11840 ahead=0 what=0
S all N=18  nb=257   lat=0 | <0,40,1,1,1,1,0,0,1> wg=257 lds=11840 ahead=0 what=0
S all N=41  nb=1     lat=0 | <0,40,1,1,1,1,0,0,1> wg=1 lds=19600 ahead=0 what=0
S all N=41  nb=256   lat=0 | <0,40,1,1,1,1,0,0,1> wg=256 lds=19600 ahead=0 what=0
S all N=41  nb=257   lat=0 | <0,40,1,1,1,1,0,0,1> wg=257 lds=19600 ahead=0 what=0
S all N=42  nb=1     lat=0 | <0,40,1,1,1,1,0,0,1> wg=1 lds=19600 ahead=0 what=0
S all N=42  nb=256   lat=0 | <0,40,1,1,1,1,0,0,1> wg=256 lds=19600 ahead=0 what=0
S all N=42  nb=257   lat=0 | <0,40,1,1,1,1,0,0,1> wg=257 lds=19600 ahead=0 what=0
S all N=65  nb=1     lat=0 | <0,40,1,1,1,1,0,0,1> wg=1 lds=19600 ahead=0 what=0
S all N=65  nb=256   lat=0 | <0,40,1,1,1,1,0,0,1> wg=256 lds=19600 ahead=0 what=0
S all N=65  nb=257   lat=0 | <0,40,1,1,1,1,0,0,1> wg=257 lds=19600 ahead=0 what=0
S all N=66  nb=1     lat=0 | <0,40,1,1,1,1,0,0,1> wg=1 lds=19600 ahead=0 what=0
S all N=66  nb=256   lat=0 | <0,40,1,1,1,1,0,0,1> wg=256 lds=19600 ahead=0 what=0
S all N=66  nb=257   lat=0 | <0,40,1,1,1,1,0,0,1> wg=257 lds=19600 ahead=0 what=0
S all N=81  nb=1     lat=0 | <0,40,1,1,1,1,0,0,1> wg=1 lds=19600 ahead=0 what=0
S all N=81  nb=256   lat=0 | <0,40,1,1,1,1,0,0,1> wg=256 lds=19600 ahead=0 what=0
S all N=81  nb=257   lat=0 | <0,40,1,1,1,1,0,0,1> wg=257 lds=19600 ahead=0 what=0
S all N=82  nb=1     lat=0 | <0,40,1,1,1,1,0,0,1> wg=1 lds=19600 ahead=0 what=0
S all N=82  nb=256   lat=0 | <0,40,1,1,1,1,0,0,1> wg=256 lds=19600 ahead=0 what=0
S all N=82  nb=257   lat=0 | <0,40,1,1,1,1,0,0,1> wg=257 lds=19600 ahead=0 what=0
S all N=130 nb=1     lat=0 | <0,40,1,1,1,1,0,0,1> wg=1 lds=19600 ahead=0 what=0
S all N=130 nb=256   lat=0 | <0,40,1,1,1,1,0,0,1> wg=256 lds=19600 ahead=0 what=0
S all N=130 nb=257   lat=0 | <0,40,1,1,1,1,0,0,1> wg=257 lds=19600 ahead=0 what=0
S fc  N=2   nb=1     lat=0 | <5,40,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
S fc  N=2   nb=256   lat=0 | <5,40,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
S fc  N=2   nb=257   lat=0 | <5,40,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
S fc  N=17  nb=1     lat=0 | <5,40,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
S fc  N=17  nb=256   lat=0 | <5,40,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
S fc  N=17  nb=257   lat=0 | <5,40,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
S fc  N=18  nb=1     lat=0 | <5,40,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
S fc  N=18  nb=256   lat=0 | <5,40,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
S fc  N=18  nb=257   lat=0 | <5,40,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
S fc  N=41  nb=1     lat=0 | <5,40,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
S fc  N=41  nb=256   lat=0 | <5,40,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
S fc  N=41  nb=257   lat=0 | <5,40,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
S fc  N=42  nb=1     lat=0 | <8,64,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
S fc  N=42  nb=256   lat=0 | <8,64,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
S fc  N=42  nb=257   lat=0 | <8,64,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
S fc  N=65  nb=1     lat=0 | <8,64,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
S fc  N=65  nb=256   lat=0 | <8,64,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
S fc  N=65  nb=257   lat=0 | <8,64,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
S fc  N=66  nb=1     lat=0 | <5,40,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
S fc  N=66  nb=256   lat=0 | <5,40,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
S fc  N=66  nb=257   lat=0 | <5,40,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
S fc  N=81  nb=1     lat=0 | <5,40,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
S fc  N=81  nb=256   lat=0 | <5,40,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
S fc  N=81  nb=257   lat=0 | <5,40,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
S fc  N=82  nb=1     lat=0 | <8,64,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
S fc  N=82  nb=256   lat=0 | <8,64,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
S fc  N=82  nb=257   lat=0 | <8,64,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
S fc  N=130 nb=1     lat=0 | <8,64,2,1,0,0,0,0,1> wg=1 lds=0 ahead=0 what=0
S fc  N=130 nb=256   lat=0 | <8,64,2,1,0,0,0,0,1> wg=256 lds=0 ahead=0 what=0
S fc  N=130 nb=257   lat=0 | <8,64,2,1,0,0,0,0,1> wg=257 lds=0 ahead=0 what=0
D cJ  N=40  nb=5735  lat=0 | <12,64,1,1,1,0,0,0,0> wg=5735 lds=0 ahead=64 what=0
D cJ  N=40  nb=5736  lat=0 | <12,64,1,1,1,0,0,1,0> wg=5736 lds=0 ahead=64 what=0
D J   N=40  nb=5735  lat=0 | <12,64,1,0,1,0,0,0,0> wg=5735 lds=0 ahead=0 what=0
D J   N=40  nb=5736  lat=0 | <12,64,1,0,1,0,0,1,0> wg=5736 lds=0 ahead=0 what=0
D all N=40  nb=5735  lat=0 | <16,64,1,1,1,0,0,0,1> wg=5735 lds=0 ahead=64 what=6
D all N=40  nb=5736  lat=0 | <16,64,1,1,1,0,0,1,1> wg=5736 lds=0 ahead=64 what=6
S cJ  N=40  nb=24235 lat=0 | <0,40,1,1,1,1,0,0,0> wg=24235 lds=19152 ahead=0 what=0
S cJ  N=40  nb=24236 lat=0 | <0,40,1,1,1,1,0,1,0> wg=24236 lds=19152 ahead=0 what=0
S all N=40  nb=24235 lat=0 | <0,40,1,1,1,1,0,0,1> wg=24235 lds=19152 ahead=0 what=0
S all N=40  nb=24236 lat=0 | <0,40,1,1,1,1,0,1,1> wg=24236 lds=19152 ahead=0 what=0
D c   N=40  nb=91180 lat=0 | <5,40,2,1,0,0,0,0,0> wg=91180 lds=0 ahead=0 what=0
D c   N=40  nb=91181 lat=0 | <5,40,2,1,0,0,0,1,0> wg=91181 lds=0 ahead=0 what=0
S fc  N=40  nb=91180 lat=0 | <5,40,2,1,0,0,0,0,1> wg=91180 lds=0 ahead=0 what=0
S fc  N=40  nb=91181 lat=0 | <5,40,2,1,0,0,0,1,1> wg=91181 lds=0 ahead=0 what=0
S cJ  N=40  nb=300   lat=0 kt=2 | <0,40,1,1,1,1,0,0,0> wg=300 lds=17808 ahead=0 what=0
S all N=40  nb=300   lat=0 kt=2 | <0,40,1,1,1,1,0,0,1> wg=300 lds=17808 ahead=0 what=0
S cJ  N=40  nb=2     lat=1 kt=2 | <0,16,2,1,1,1,1,0,0> wg=6 lds=7312 ahead=0 what=0
S cJ  N=40  nb=300   lat=0 | <0,40,1,1,1,1,0,0,0> wg=300 lds=19152 ahead=0 what=0
S all N=40  nb=300   lat=0 | <0,40,1,1,1,1,0,0,1> wg=300 lds=19152 ahead=0 what=0
S cJ  N=40  nb=2     lat=1 | <0,16,2,1,1,1,1,0,0> wg=6 lds=8656 ahead=0 what=0
S cJ  N=40  nb=300   lat=0 kt=41 | <0,40,1,1,1,1,0,0,0> wg=300 lds=22176 ahead=0 what=0
S all N=40  nb=300   lat=0 kt=41 | <0,40,1,1,1,1,0,0,1> wg=300 lds=22176 ahead=0 what=0
S cJ  N=40  nb=2     lat=1 kt=41 | <0,16,2,1,1,1,1,0,0> wg=6 lds=9104 ahead=0 what=0
"""

TUNING = """
D c   N=41  nb=300   lat=0 var=1 | <8,64,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=1 | <8,64,2,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=1 | <8,64,2,1,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S c   N=41  nb=300   lat=0 var=1 | <8,64,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=1 | <8,64,2,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=1 | <8,64,2,1,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=2 | <12,64,1,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=2 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=2 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S c   N=41  nb=300   lat=0 var=2 | <12,64,1,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=2 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=2 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=3 | <16,64,1,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=3 | <16,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=3 | <16,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S c   N=41  nb=300   lat=0 var=3 | <16,64,1,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=3 | <16,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=3 | <16,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=4 | <12,64,1,1,0,0,0,0,0> wg=300 lds=0 ahead=64 what=0
D J   N=41  nb=300   lat=0 var=4 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=4 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=4 | <12,64,1,1,0,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S J   N=41  nb=300   lat=0 var=4 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=4 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
D c   N=41  nb=300   lat=0 var=5 | <12,64,2,1,0,0,0,0,0> wg=300 lds=0 ahead=64 what=0
D J   N=41  nb=300   lat=0 var=5 | <12,64,2,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=5 | <12,64,2,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=5 | <12,64,2,1,0,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S J   N=41  nb=300   lat=0 var=5 | <12,64,2,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=5 | <12,64,2,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
D c   N=41  nb=300   lat=0 var=6 | <10,64,2,1,0,0,0,0,0> wg=300 lds=0 ahead=64 what=0
D J   N=41  nb=300   lat=0 var=6 | <10,64,2,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=6 | <10,64,2,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=6 | <10,64,2,1,0,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S J   N=41  nb=300   lat=0 var=6 | <10,64,2,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=6 | <10,64,2,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
D c   N=41  nb=300   lat=0 var=7 | <12,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=64 what=0
D J   N=41  nb=300   lat=0 var=7 | <12,40,2,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=7 | <12,40,2,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=7 | <12,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S J   N=41  nb=300   lat=0 var=7 | <12,40,2,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=7 | <12,40,2,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
D c   N=41  nb=300   lat=0 var=8 | <8,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=64 what=0
D J   N=41  nb=300   lat=0 var=8 | <8,40,2,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=8 | <8,40,2,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=8 | <8,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S J   N=41  nb=300   lat=0 var=8 | <8,40,2,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=8 | <8,40,2,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
D c   N=41  nb=300   lat=0 var=9 | <16,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=64 what=0
D J   N=41  nb=300   lat=0 var=9 | <16,40,2,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=9 | <16,40,2,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=9 | <16,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S J   N=41  nb=300   lat=0 var=9 | <16,40,2,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=9 | <16,40,2,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
D c   N=41  nb=300   lat=0 var=10 | <10,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=64 what=0
D J   N=41  nb=300   lat=0 var=10 | <10,40,2,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=10 | <10,40,2,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=10 | <10,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S J   N=41  nb=300   lat=0 var=10 | <10,40,2,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=10 | <10,40,2,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
D c   N=41  nb=300   lat=0 var=11 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=11 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=11 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=11 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=11 | <0,32,2,0,1,1,0,0,0> wg=300 lds=15952 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=11 | <0,32,2,1,1,1,0,0,0> wg=300 lds=15952 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=12 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=12 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=12 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=12 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=12 | <0,40,2,0,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=12 | <0,40,2,1,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=13 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=13 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=13 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=13 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=13 | <0,32,1,0,1,1,0,0,0> wg=300 lds=15952 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=13 | <0,32,1,1,1,1,0,0,0> wg=300 lds=15952 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=14 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=14 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=14 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=14 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=14 | <0,64,1,0,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=14 | <0,64,1,1,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=15 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=15 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=15 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=15 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=15 | <0,64,2,0,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=15 | <0,64,2,1,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=16 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=16 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=16 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=16 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=16 | <20,40,3,0,1,1,0,0,0> wg=300 lds=11328 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=16 | <20,40,3,1,1,1,0,0,0> wg=300 lds=11328 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=17 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=17 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=17 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=17 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=17 | <20,40,2,0,1,1,0,0,0> wg=300 lds=11328 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=17 | <20,40,2,1,1,1,0,0,0> wg=300 lds=11328 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=18 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=18 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=18 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=18 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=18 | <0,40,2,0,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=18 | <0,40,2,1,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=19 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=19 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=19 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=19 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=19 | <14,40,3,0,1,1,0,0,0> wg=300 lds=11328 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=19 | <14,40,3,1,1,1,0,0,0> wg=300 lds=11328 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=21 | <16,16,1,1,0,0,1,0,0> wg=900 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=21 | <16,16,1,0,1,0,1,0,0> wg=900 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=21 | <16,16,1,1,1,0,1,0,0> wg=900 lds=0 ahead=0 what=0
S c   N=41  nb=300   lat=0 var=21 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=21 | <0,40,1,0,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=21 | <0,40,1,1,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=22 | <8,8,2,1,0,0,1,0,0> wg=1500 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=22 | <8,8,2,0,1,0,1,0,0> wg=1500 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=22 | <8,8,2,1,1,0,1,0,0> wg=1500 lds=0 ahead=0 what=0
S c   N=41  nb=300   lat=0 var=22 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=22 | <0,40,1,0,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=22 | <0,40,1,1,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=23 | <10,10,2,1,0,0,1,0,0> wg=1200 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=23 | <10,10,2,0,1,0,1,0,0> wg=1200 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=23 | <10,10,2,1,1,0,1,0,0> wg=1200 lds=0 ahead=0 what=0
S c   N=41  nb=300   lat=0 var=23 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=23 | <0,40,1,0,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=23 | <0,40,1,1,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=24 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=24 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=24 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=24 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=24 | <0,16,2,0,1,1,1,0,0> wg=900 lds=8656 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=24 | <0,16,2,1,1,1,1,0,0> wg=900 lds=8656 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=25 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=25 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=25 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=25 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=25 | <0,8,2,0,1,1,1,0,0> wg=1500 lds=4560 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=25 | <0,8,2,1,1,1,1,0,0> wg=1500 lds=4560 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=31 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=31 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=31 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=31 | <5,40,2,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=31 | <0,40,1,0,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=31 | <0,40,1,1,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=32 | <5,40,3,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=32 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=32 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=32 | <5,40,3,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=32 | <0,40,1,0,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=32 | <0,40,1,1,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=33 | <5,40,4,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=33 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=33 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=33 | <5,40,4,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=33 | <0,40,1,0,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=33 | <0,40,1,1,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=34 | <8,64,3,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=34 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=34 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=34 | <8,64,3,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=34 | <0,40,1,0,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=34 | <0,40,1,1,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=35 | <8,64,4,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=35 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=35 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=35 | <8,64,4,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=35 | <0,40,1,0,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=35 | <0,40,1,1,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=36 | <4,32,3,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=36 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=36 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=36 | <4,32,3,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=36 | <0,40,1,0,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=36 | <0,40,1,1,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
D c   N=41  nb=300   lat=0 var=37 | <4,32,4,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D J   N=41  nb=300   lat=0 var=37 | <12,64,1,0,1,0,0,0,0> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=300   lat=0 var=37 | <12,64,1,1,1,0,0,0,0> wg=300 lds=0 ahead=64 what=0
S c   N=41  nb=300   lat=0 var=37 | <4,32,4,1,0,0,0,0,0> wg=300 lds=0 ahead=0 what=0
S J   N=41  nb=300   lat=0 var=37 | <0,40,1,0,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
S cJ  N=41  nb=300   lat=0 var=37 | <0,40,1,1,1,1,0,0,0> wg=300 lds=19600 ahead=0 what=0
S cJ  N=41  nb=2     lat=1 var=11 | <0,16,2,1,1,1,1,0,0> wg=6 lds=8656 ahead=0 what=0
D all N=41  nb=300   lat=0 var=5 | <16,64,1,1,1,0,0,0,1> wg=300 lds=0 ahead=64 what=6
D fc  N=41  nb=300   lat=0 var=33 | <5,40,2,1,0,0,0,0,1> wg=300 lds=0 ahead=0 what=0
D cJ  N=41  nb=2     lat=0 env=16,-1,0 | <12,64,1,1,1,0,0,0,0> wg=2 lds=0 ahead=16 what=0
D c   N=41  nb=2     lat=0 env=16,-1,0 | <5,40,2,1,0,0,0,0,0> wg=2 lds=0 ahead=16 what=0
D J   N=41  nb=2     lat=0 env=16,-1,0 | <12,64,1,0,1,0,0,0,0> wg=2 lds=0 ahead=16 what=0
S cJ  N=41  nb=2     lat=0 env=16,-1,0 | <0,40,1,1,1,1,0,0,0> wg=2 lds=19600 ahead=16 what=0
D all N=41  nb=2     lat=0 env=16,-1,0 | <16,64,1,1,1,0,0,0,1> wg=2 lds=0 ahead=16 what=6
D fc  N=41  nb=2     lat=0 env=16,-1,0 | <5,40,2,1,0,0,0,0,1> wg=2 lds=0 ahead=0 what=0
D cJ  N=41  nb=2     lat=1 env=16,-1,0 | <16,16,1,1,1,0,1,0,0> wg=6 lds=0 ahead=0 what=0
D cJ  N=41  nb=2     lat=0 env=-1,6,0 | <12,64,1,1,1,0,0,0,0> wg=2 lds=0 ahead=64 what=7
D c   N=41  nb=2     lat=0 env=-1,6,0 | <5,40,2,1,0,0,0,0,0> wg=2 lds=0 ahead=0 what=7
D J   N=41  nb=2     lat=0 env=-1,6,0 | <12,64,1,0,1,0,0,0,0> wg=2 lds=0 ahead=0 what=7
S cJ  N=41  nb=2     lat=0 env=-1,6,0 | <0,40,1,1,1,1,0,0,0> wg=2 lds=19600 ahead=0 what=7
D all N=41  nb=2     lat=0 env=-1,6,0 | <16,64,1,1,1,0,0,0,1> wg=2 lds=0 ahead=64 what=7
D fc  N=41  nb=2     lat=0 env=-1,6,0 | <5,40,2,1,0,0,0,0,1> wg=2 lds=0 ahead=0 what=0
D cJ  N=41  nb=2     lat=1 env=-1,6,0 | <16,16,1,1,1,0,1,0,0> wg=6 lds=0 ahead=0 what=0
D cJ  N=41  nb=2     lat=0 env=128,7,4096 | <12,64,1,1,1,0,0,0,0> wg=2 lds=4096 ahead=128 what=6
D c   N=41  nb=2     lat=0 env=128,7,4096 | <5,40,2,1,0,0,0,0,0> wg=2 lds=0 ahead=128 what=6
D J   N=41  nb=2     lat=0 env=128,7,4096 | <12,64,1,0,1,0,0,0,0> wg=2 lds=0 ahead=128 what=6
S cJ  N=41  nb=2     lat=0 env=128,7,4096 | <0,40,1,1,1,1,0,0,0> wg=2 lds=23696 ahead=128 what=6
D all N=41  nb=2     lat=0 env=128,7,4096 | <16,64,1,1,1,0,0,0,1> wg=2 lds=0 ahead=128 what=6
D fc  N=41  nb=2     lat=0 env=128,7,4096 | <5,40,2,1,0,0,0,0,1> wg=2 lds=0 ahead=0 what=0
D cJ  N=41  nb=2     lat=1 env=128,7,4096 | <16,16,1,1,1,0,1,0,0> wg=6 lds=4096 ahead=0 what=0
D cJ  N=41  nb=2     lat=0 env=0,0,0 | <12,64,1,1,1,0,0,0,0> wg=2 lds=0 ahead=0 what=1
D c   N=41  nb=2     lat=0 env=0,0,0 | <5,40,2,1,0,0,0,0,0> wg=2 lds=0 ahead=0 what=1
D J   N=41  nb=2     lat=0 env=0,0,0 | <12,64,1,0,1,0,0,0,0> wg=2 lds=0 ahead=0 what=1
S cJ  N=41  nb=2     lat=0 env=0,0,0 | <0,40,1,1,1,1,0,0,0> wg=2 lds=19600 ahead=0 what=1
D all N=41  nb=2     lat=0 env=0,0,0 | <16,64,1,1,1,0,0,0,1> wg=2 lds=0 ahead=0 what=1
D fc  N=41  nb=2     lat=0 env=0,0,0 | <5,40,2,1,0,0,0,0,1> wg=2 lds=0 ahead=0 what=0
D cJ  N=41  nb=2     lat=1 env=0,0,0 | <16,16,1,1,1,0,1,0,0> wg=6 lds=0 ahead=0 what=0
"""


def _request(left):
    """'D cJ N=41 nb=256 lat=0 kt=2 var=11 env=16,-1,0' -> the program's input line"""
    tok = left.split()
    kv = dict(t.split("=") for t in tok[2:])
    out = tok[1]
    c, vals = int(out in ("c", "cJ", "all", "fc")), int(out in ("J", "cJ", "all"))
    f, grad = int(out in ("all", "fc")), int(out == "all")
    env = kv.get("env", "-1,-1,0").split(",")
    return " ".join(str(v) for v in (kv["nb"], kv["N"], {"D": 0, "S": 1}[tok[0]], kv.get("kt", 14), c, vals, f, grad, kv["lat"],
                                     kv.get("var", 0), *env))


def _check(tmp_path, table, *defines):
    exe = str(tmp_path / "launch_plan_print")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "--offload-host-only", "--offload-arch=gfx950", "-Wall", "-Wextra", "-Werror", *defines,
                    "-o", exe, os.path.join(ROOT, "tests", "launch_plan_print.cpp")], check=True)
    lines = [l for l in table.strip().splitlines()]
    left = [l.split("|")[0].strip() for l in lines]
    want = [re.sub(r"\s+", " ", l.split("|")[1].strip()) for l in lines]
    out = subprocess.run([exe], input="\n".join(_request(l) for l in left) + "\n", capture_output=True, text=True, check=True)
    got = [re.sub(r" flags=\d+$", "", l) for l in out.stdout.splitlines()]
    assert len(got) == len(want)
    wrong = [f"{l}: want {w}, got {g}" for l, w, g in zip(left, want, got) if w != g]
    assert not wrong, "\n".join(wrong)
    # the flags word: QLN_JAC_WRITE_CONSTANTS in bit 0, the distance from bit 8, what is prefetched in bits 29..31
    for l, w in zip(out.stdout.splitlines(), want):
        ahead, what = (int(x) for x in re.search(r"ahead=(\d+) what=(\d+)", w).groups())
        assert int(l.rsplit("flags=", 1)[1]) == 1 | (ahead << 8) | (what << 29)
    return len(want)


def test_product_plan_matches_the_table(tmp_path):
    assert _check(tmp_path, PRODUCT) == 503


def test_tuning_variants_match_the_table(tmp_path):
    assert _check(tmp_path, TUNING, "-DQLN_TUNING") == 217
