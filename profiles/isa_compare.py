"""Instruction-for-instruction comparison of the gfx950 kernels of two revisions (no GPU needed):

    python profiles/isa_compare.py [REV]          # REV defaults to HEAD; the working tree is the other side

Both sides are compiled to assembly with the flags of balloon_learning_environment_amd/_lib.py::build (hipcc -S --cuda-device-only),
every kernel's body is cut out of the two .s files by its symbol, and the bodies of the kernels present on both sides are compared
line by line (comments and blank lines dropped; the function's ordinal in its local labels, .LBB<ordinal>_<block>, is dropped too: it
counts the functions emitted before this one, so a kernel added to the file renumbers the labels of every later one without changing
an instruction).  Prints one line per kernel and exits 1 if any common kernel differs.  Kernels present
on one side only are listed, not compared -- except those a new trailing template parameter renamed: a kernel of REV whose demangled
name equals a kernel's of the tree once that one's trailing `false` template arguments (and the empty parameter pack behind them)
are dropped is compared with it, body against body (the lines that carry the symbol itself aside), and reported as `renamed`."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assemble(tree: str, out: str) -> str:
  src = os.path.join(tree, 'balloon_learning_environment_amd', 'csrc')
  subprocess.check_call(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=on', '-fPIC', '-I', src, '-S',
                         '--cuda-device-only', '-o', out, os.path.join(src, 'ble_kernels.hip')])
  return open(out).read()


def kernels(asm: str) -> dict:
  """{symbol: [instruction lines]} of every function with a .type ...,@function"""
  out = {}
  for name in re.findall(r'^\s*\.type\s+(\S+),@function', asm, re.M):
    start = re.search(r'^' + re.escape(name) + r':', asm, re.M)
    end = re.search(r'^\.Lfunc_end\d+:', asm[start.end():], re.M)
    body = asm[start.end():start.end() + end.start()]
    lines = []
    for line in body.splitlines():
      line = line.split(';')[0].rstrip()
      if line.strip():
        lines.append(re.sub(r'\.(LBB|LJTI|LCPI)\d+_', r'.\1_', line.strip()))
    out[name] = lines
  return out


def demangle(names):
  return subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.splitlines() if names else []


def short_name(demangled: str) -> str:
  """The kernel's name with its template arguments, without its parameter list."""
  return re.sub(r'^void ', '', demangled.split('(')[0])


def main() -> int:
  rev = sys.argv[1] if len(sys.argv) > 1 else 'HEAD'
  with tempfile.TemporaryDirectory() as tmp:
    base = os.path.join(tmp, 'base')
    os.makedirs(base)
    archive = subprocess.check_output(['git', '-C', ROOT, 'archive', rev, 'balloon_learning_environment_amd/csrc', 'include'])
    subprocess.run(['tar', 'x', '-C', base], input=archive, check=True)
    a = kernels(assemble(base, os.path.join(tmp, 'base.s')))
    b = kernels(assemble(ROOT, os.path.join(tmp, 'tree.s')))
  differ = 0
  for name in sorted(set(a) & set(b)):
    same = a[name] == b[name]
    differ += not same
    print(f'{"identical" if same else "DIFFERS  "} {len(a[name]):6d} / {len(b[name]):6d} lines  {name}')
  only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
  old_name = {short_name(d): n for n, d in zip(only_a, demangle(only_a))}
  renamed = 0
  for name, d in zip(only_b, demangle(only_b)):
    d = short_name(d)
    while d not in old_name and re.search(r', false>', d):
      d = re.sub(r', false>', '>', d, count=1)
    if d in old_name:
      old = old_name.pop(d)
      strip = lambda lines, sym: [l for l in lines if sym not in l]
      same = strip(a[old], old) == strip(b[name], name)
      differ += not same
      renamed += 1
      print(f'{"identical" if same else "DIFFERS  "} {len(a[old]):6d} / {len(b[name]):6d} lines  renamed: {d}')
    else:
      print(f'only in the tree: {name}')
  for name in old_name.values():
    print(f'only in {rev}: {name}')
  print(f'{len(set(a) & set(b)) + renamed - differ} of {len(set(a) & set(b))} common and {renamed} renamed kernels identical')
  return 1 if differ else 0


if __name__ == '__main__':
  sys.exit(main())
