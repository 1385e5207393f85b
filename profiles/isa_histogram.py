"""Instruction-class histogram of the fused step kernel's stride loop and of its per-step part (no GPU needed):

    python profiles/isa_histogram.py [REV ...] [--kernel SUBSTRING] [--dump | --dump-step | --dump-helper] [--cost]

Every REV (a git revision; `tree` = the working tree, the default) is compiled to gfx950 assembly with the flags of
balloon_learning_environment_amd/_lib.py::build (profiles/isa_compare.py::assemble), the kernel whose symbol contains SUBSTRING
(default: ble_step_kernel<false, VehicleDefault>) is cut out, and its loops are found:

  * the STRIDE LOOP is the innermost loop with the most fp64 instructions: two strides per iteration (ble_step_core.h);
  * the STEP LOOP is the smallest loop that contains it: one agent step per iteration.

Both are reduced to their HOT PATH: the blocks a wave runs when no rare path is taken (hot_path below: unconditional jumps are
followed; a conditional branch only where it skips a block left in line; rare blocks placed out of line -- `if (wave_any(c)) if (c)` --
and loop exits are not).  The per-step part is the step loop's hot path without the stride loop and without the third, in-line copy of
the stride (`if (ks < substeps) stride(ks)`: an even `substeps` never runs it).  The loops are taken from the compiler's own block
comments (`Loop Header`, `in Loop: Header=`): a profiling aid for this compiler, not a disassembler.  One table per revision, one column
per part, the stride loop also per stride; --dump (--dump-step) prints the hot path of the stride loop (of the per-step part) with its line numbers in the .s file (kept in
the temporary directory as isa_histogram_<rev>.s) for attribution to the
source.

A kernel with a helper wave (--kernel ble_step_helper_kernel, csrc/ble_step_helper.h) holds TWO role loops.  The main wave's are found as
above (its stride carries the fp64).  The helper wave's step loop is the other outermost loop of the kernel, and its record loop -- one
SunRecord per iteration, i.e. per stride -- the loop inside it with the most instructions (the others are the polling loops of the
hand-over, a handful of instructions each).  A second table gives the helper's record loop and per-step part.

--cost weights the hot paths with the issue costs of profiles/r02_microbench.md (`valu_op_cost`, ns per wave instruction) and prints them
per stride and per agent step (18 strides + the per-step part) in two columns:
  * ONE WAVE: what a wave alone on its SIMD needs to issue the path -- 2.1 ns per instruction of any kind, 7.0 for an fp64 seed
    (v_rcp / v_rsq / v_sqrt_f64), 4.15 for an fp32 transcendental, 3.1 for a conversion to or from fp64;
  * TWO WAVES: the VALU pipe time of the path when a second wave shares the SIMD -- 2.05 ns per fp64 instruction, 6.85 per fp64 seed, 3.5 per
    fp32 transcendental, 1.6 per conversion to or from fp64, 1.05 per other vector instruction; scalar instructions, branches, waits, LDS
    and memory instructions do not occupy the pipe.
With a helper wave the two-waves column also gets the sum over both waves: the pipe time M and S need together per stride and per step."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_compare import ROOT, assemble  # noqa: E402

DEFAULT_KERNEL = 'ble_step_kernelILb0EN3ble14VehicleDefaultEEE'
CLASSES = ['fp64 arithmetic', 'fp32 arithmetic', 'v_cmp*', 'v_cndmask*', 'v_cvt*', 'other vector', 'moves', 'LDS', 'memory', 'SALU',
           'branches', 'waits', 's_nop']


def classify(op: str) -> str:
  if op.startswith('v_cmp'):
    return 'v_cmp*'
  if op.startswith('v_cndmask'):
    return 'v_cndmask*'
  if op.startswith('v_cvt'):
    return 'v_cvt*'
  if op.startswith(('v_mov', 'v_accvgpr', 'v_readfirstlane', 'v_readlane', 'v_writelane', 'v_swap')):
    return 'moves'
  if op.startswith('v_'):
    if '_f64' in op:
      return 'fp64 arithmetic'
    if '_f32' in op or '_f16' in op:
      return 'fp32 arithmetic'
    return 'other vector'
  if op.startswith('ds_'):
    return 'LDS'
  if op.startswith(('global_', 'buffer_', 'flat_', 'scratch_', 's_load', 's_buffer_load')):
    return 'memory'
  if op.startswith('s_waitcnt') or op.startswith('s_wait'):
    return 'waits'
  if op == 's_nop':
    return 's_nop'
  if op.startswith(('s_cbranch', 's_branch')):
    return 'branches'
  return 'SALU'


def kernel_body(asm: str, key: str):
  """[(line number in the .s file, text, loop)] of the kernel whose symbol contains `key`: labels and instructions; `loop` is the header
  label of the innermost loop the line's block belongs to (the compiler's own block comments), and parents[header] the loop around it"""
  lines = asm.splitlines()
  start = next(i for i, l in enumerate(lines) if re.match(r'^\S*' + re.escape(key) + r'\S*:', l))
  out, parents, loop = [], {}, None
  for i in range(start + 1, len(lines)):
    if re.match(r'^\.Lfunc_end\d+:', lines[i]):
      break
    text, _, comment = lines[i].partition(';')
    text = text.strip()
    label = re.match(r'^(\.LBB\d+_\d+):', text)
    if label or re.match(r'^\s*; %bb\.\d+:', lines[i]):           # a new block: its loop, from the comment (none: outside every loop)
      block_comment = lines[i]
      for j in range(i + 1, min(i + 4, len(lines))):               # (a header's comment goes on over the next lines)
        if not lines[j].lstrip().startswith(';') or '%bb.' in lines[j]:
          break
        block_comment += lines[j]
      m = re.search(r'in Loop: Header=(BB\d+_\d+)', block_comment)
      if m:
        loop = '.L' + m.group(1)
      elif 'Loop Header' in block_comment and label:
        loop = label.group(1)
        m = re.findall(r'Parent Loop (BB\d+_\d+)', block_comment)
        parents[loop] = '.L' + m[-1] if m else None
      else:
        loop = None
    if text and (label or not text.startswith('.')):
      out.append((i + 1, text, loop))
  return lines[start].split(':')[0], out, parents


def in_loop(loop, header, parents) -> bool:
  while loop is not None:
    if loop == header:
      return True
    loop = parents.get(loop)
  return False


def hot_path(body, parents, header, inner=None):
  """indices of the instructions a wave runs from the loop's header back to it when no rare path is taken.  Unconditional jumps are
  followed.  A conditional branch is followed only if it skips a block left in line: target inside the loop, further down, reached by
  fall-through too; not followed are loop exits and rare blocks placed out of line (`if (wave_any(c)) if (c)`: an unconditional jump
  stands in front of them).  `inner`: the header of an inner loop that is left out (the walk goes on at its exit, past the odd last stride)."""
  label_at = {t[:-1]: k for k, (_, t, _) in enumerate(body) if t.endswith(':')}
  k, path, seen, after_inner = label_at[header], [], set(), False
  while True:
    if k in seen:                        # (a cycle that does not pass the header: the walk ends where it closes)
      return path
    seen.add(k)
    _, t, loop = body[k]
    if inner and t == inner + ':':       # the inner loop: on to the target of its exit branch
      k = next(label_at[m.group(1)] for j in range(k, len(body)) if body[j][2] == inner
               for m in [re.match(r'^s_cbranch\S*\s+(\.LBB\d+_\d+)', body[j][1])] if m and not in_loop(body[label_at[m.group(1)]][2], inner, parents))
      after_inner = True
      continue
    if not t.endswith(':'):
      path.append(k)
      m = re.match(r'^s_(c?)branch\S*\s+(\.LBB\d+_\d+)', t)
      if m:
        target = label_at[m.group(2)]
        if m.group(2) == header:        # the back edge
          return path
        if m.group(1) == '':
          k = target
          continue
        if after_inner and t.startswith('s_cbranch_scc'):
          # the exit block of the inner loop closes with the guard of the odd last stride (`if (ks < substeps) stride(ks)`, a third copy of
          # the stride that an even `substeps` never runs): a scalar condition, followed wherever the compiler put its target
          after_inner = False
          k = target
          continue
        over_inner = inner is not None and k < label_at[inner] < target      # (`if (live)`: it skips the whole step)
        if target > k and not over_inner and in_loop(body[target][2], header, parents) and not re.match(r'^s_branch\b', body[target - 1][1]):
          k = target
          continue
    k += 1


SEEDS_F64 = ('v_rcp_f64', 'v_rsq_f64', 'v_sqrt_f64')
TRANS_F32 = ('v_exp_f32', 'v_log_f32', 'v_rcp_f32', 'v_rsq_f32', 'v_sqrt_f32', 'v_sin_f32', 'v_cos_f32', 'v_rcp_iflag_f32')
COST_ROWS = ['fp64 seeds', 'fp32 transcendentals', 'conversions to / from fp64', 'other fp64', 'other vector', 'not on the VALU pipe']
COST_NS = {'fp64 seeds': (7.0, 6.85), 'fp32 transcendentals': (4.15, 3.5), 'conversions to / from fp64': (3.1, 1.6), 'other fp64': (2.1, 2.05),
           'other vector': (2.1, 1.05), 'not on the VALU pipe': (2.1, 0.0)}       # (one wave per SIMD, two waves per SIMD)


def cost_class(op: str) -> str:
  base = op.split('_e32')[0].split('_e64')[0].split('_sdwa')[0].split('_dpp')[0]
  if base in SEEDS_F64:
    return 'fp64 seeds'
  if base in TRANS_F32:
    return 'fp32 transcendentals'
  if op.startswith('v_cvt') and 'f64' in op:
    return 'conversions to / from fp64'
  if op.startswith('v_'):
    return 'other fp64' if ('_f64' in op or '_b64' in op) else 'other vector'
  return 'not on the VALU pipe'


def cost(body, path):
  """{row: (count, ns one wave, ns two waves)} of a hot path, and the totals"""
  rows = {r: [0, 0.0, 0.0] for r in COST_ROWS}
  for k in path:
    r = cost_class(body[k][1].split()[0])
    rows[r][0] += 1; rows[r][1] += COST_NS[r][0]; rows[r][2] += COST_NS[r][1]
  return rows, sum(v[1] for v in rows.values()), sum(v[2] for v in rows.values())


def report_cost(title, body, stride_path, strides_per_iteration, step_path):
  """the cost-weighted hot path per stride and per agent step (18 strides + the per-step part); returns (one wave, two waves) per step"""
  rs, s1, s2 = cost(body, stride_path)
  rp, p1, p2 = cost(body, step_path)
  d = float(strides_per_iteration)
  print(f'{title}: cost-weighted hot path (ns; `valu_op_cost` of r02_microbench.md)')
  print('| Class | Per stride: count | one wave | two waves | Per-step part: count | one wave | two waves |')
  print('|---|---|---|---|---|---|---|')
  for r in COST_ROWS:
    print(f'| {r} | {rs[r][0] / d:g} | {rs[r][1] / d:.1f} | {rs[r][2] / d:.1f} | {rp[r][0]} | {rp[r][1]:.1f} | {rp[r][2]:.1f} |')
  print(f'| **all** | {len(stride_path) / d:g} | {s1 / d:.1f} | {s2 / d:.1f} | {len(step_path)} | {p1:.1f} | {p2:.1f} |')
  step1, step2 = 18 * s1 / d + p1, 18 * s2 / d + p2
  print(f'per agent step (18 strides + the per-step part): one wave {step1 / 1e3:.2f} us, two waves (pipe time) {step2 / 1e3:.2f} us')
  print()
  return step1, step2


def histogram(body, path):
  h = dict.fromkeys(CLASSES, 0)
  for k in path:
    h[classify(body[k][1].split()[0])] += 1
  return h


def analyse(asm: str, key: str):
  name, body, parents = kernel_body(asm, key)
  f64 = {}
  for _, t, loop in body:
    if loop and '_f64' in t.split()[0]:
      f64[loop] = f64.get(loop, 0) + 1
  # the innermost loop with the most fp64 work on its hot path (a rare fp64 chain kept inside another loop -- the helper wave's sun_exact --
  # does not count); polling loops of a hand-over inside it (ble_step_helper.h: a few instructions, no fp64,
  # behind a branch the hot path does not take) do not make it an outer loop
  size = {}
  for _, t, loop in body:
    if loop and not t.endswith(':'):
      size[loop] = size.get(loop, 0) + 1
  def innermost(l):
    return all(size.get(c, 0) < 30 and c not in f64 for c, p in parents.items() if p == l)
  def hot_f64(l):
    return sum('_f64' in body[k][1].split()[0] for k in hot_path(body, parents, l))
  stride = max((l for l in f64 if innermost(l)), key=hot_f64)
  step = parents[stride]
  return name, body, hot_path(body, parents, stride), hot_path(body, parents, step, inner=stride)


def analyse_helper_role(body, parents, main_step):
  """(record loop's hot path, per-step hot path) of the helper wave: the loops outside the main wave's step loop; None if there are none"""
  size = {}
  for _, t, loop in body:
    if loop and not t.endswith(':'):
      size[loop] = size.get(loop, 0) + 1
  def root(l):
    while parents.get(l) is not None:
      l = parents[l]
    return l
  total = {}
  for l, v in size.items():
    if root(l) != root(main_step):
      total[root(l)] = total.get(root(l), 0) + v
  if not total:
    return None
  step = max(total, key=total.get)
  inner = [l for l in size if l != step and in_loop(l, step, parents)]
  if not inner:
    return None
  record = max(inner, key=size.get)
  return hot_path(body, parents, record), hot_path(body, parents, step, inner=record)


def report_helper_role(body, record_path, step_path, with_cost=False):
  hr, hp = histogram(body, record_path), histogram(body, step_path)
  print(f'helper wave: record loop .s lines {body[record_path[0]][0]}-{body[record_path[-1]][0]} (one record = one stride per iteration)')
  print('| Class | Per record (stride) | Per-step part |')
  print('|---|---|---|')
  for c in CLASSES:
    print(f'| {c} | {hr[c]} | {hp[c]} |')
  print(f'| **all** | {len(record_path)} | {len(step_path)} |')
  vec = lambda h: sum(v for c, v in h.items() if c in CLASSES[:9])
  print(f'vector (incl. LDS, memory) / scalar per record: {vec(hr)} / {len(record_path) - vec(hr)}; per-step part: {vec(hp)} / {len(step_path) - vec(hp)}')
  print()
  return report_cost('helper wave', body, record_path, 1, step_path) if with_cost else None


def report(rev: str, asm: str, key: str, dump: bool, with_cost: bool = False) -> None:
  name, body, stride_path, step_path = analyse(asm, key)
  hs, hp = histogram(body, stride_path), histogram(body, step_path)
  print(f'## {rev}: {name[:90]}')
  print(f'stride loop: .s lines {body[stride_path[0]][0]}-{body[stride_path[-1]][0]}; the per-step part is scattered over {len({body[k][2] for k in step_path})} loop levels of .s lines {min(body[k][0] for k in step_path)}-{max(body[k][0] for k in step_path)}')
  print('| Class | Per two strides | Per stride | Per-step part |')
  print('|---|---|---|---|')
  for c in CLASSES:
    print(f'| {c} | {hs[c]} | {hs[c] / 2:g} | {hp[c]} |')
  print(f'| **all** | {len(stride_path)} | {len(stride_path) / 2:g} | {len(step_path)} |')
  vec = lambda h: sum(v for c, v in h.items() if c in CLASSES[:9])
  print(f'vector (incl. LDS, memory) / scalar per two strides: {vec(hs)} / {len(stride_path) - vec(hs)}; per-step part: {vec(hp)} / {len(step_path) - vec(hp)}')
  print()
  main_cost = report_cost('main wave', body, stride_path, 2, step_path) if with_cost else None
  _, _, parents = kernel_body(asm, key)
  helper = analyse_helper_role(body, parents, body[step_path[0]][2] if body[step_path[0]][2] else None) if 'helper' in name else None
  if helper:
    helper_cost = report_helper_role(body, *helper, with_cost=with_cost)
    if with_cost:
      print(f'both waves, pipe time per agent step (two-waves column, main + helper): {(main_cost[1] + helper_cost[1]) / 1e3:.2f} us')
      print()
    if dump == 'helper':
      for k in helper[0]:
        print(f'{body[k][0]:7d}  {classify(body[k][1].split()[0]):16s} {body[k][1]}')
  if dump:
    for k in (step_path if dump == 'step' else stride_path):
      print(f'{body[k][0]:7d}  {classify(body[k][1].split()[0]):16s} {body[k][1]}')


def main() -> int:
  args = sys.argv[1:]
  dump = 'step' if '--dump-step' in args else ('helper' if '--dump-helper' in args else '--dump' in args)
  key = DEFAULT_KERNEL
  if '--kernel' in args:
    key = args[args.index('--kernel') + 1]
    del args[args.index('--kernel'):args.index('--kernel') + 2]
  with_cost = '--cost' in args
  revs = [a for a in args if not a.startswith('--')] or ['tree']
  with tempfile.TemporaryDirectory() as tmp:
    for rev in revs:
      tree = ROOT
      if rev.endswith('.s'):             # an assembly file made earlier
        report(rev, open(rev).read(), key, dump, with_cost)
        continue
      if rev != 'tree':
        tree = os.path.join(tmp, re.sub(r'\W', '_', rev))
        os.makedirs(tree)
        archive = subprocess.check_output(['git', '-C', ROOT, 'archive', rev, 'balloon_learning_environment_amd/csrc', 'include'])
        subprocess.run(['tar', 'x', '-C', tree], input=archive, check=True)
      out = os.path.join(tempfile.gettempdir(), 'isa_histogram_' + re.sub(r'\W', '_', rev) + '.s')
      report(rev, assemble(tree, out), key, dump, with_cost)
  return 0


if __name__ == '__main__':
  sys.exit(main())
