"""Instruction-for-instruction comparison of the gfx950 kernels of two revisions (no GPU needed):

    python profiles/isa_compare.py [REV]          # REV defaults to HEAD; the working tree is the other side

Both sides are compiled to assembly with the flags of balloon_learning_environment_amd/_lib.py::build (hipcc -S --cuda-device-only),
every kernel's body is cut out of the two .s files by its symbol, and the bodies of the kernels present on both sides are compared
line by line (comments and blank lines dropped; the function's ordinal in its local labels, .LBB<ordinal>_<block>, is dropped too: it
counts the functions emitted before this one, so a kernel added to the file renumbers the labels of every later one without changing
an instruction).  Prints one line per kernel and exits 1 if any common kernel differs.  Kernels present
on one side only are listed, not compared."""
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
  for name in sorted(set(a) ^ set(b)):
    print(f'only in {"the tree" if name in b else rev}: {name}')
  print(f'{len(set(a) & set(b)) - differ} of {len(set(a) & set(b))} common kernels identical')
  return 1 if differ else 0


if __name__ == '__main__':
  sys.exit(main())
