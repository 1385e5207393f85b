"""Evaluation suites (eval/suites.py of the reference): which seeds an agent is evaluated on, and for how many steps."""
import dataclasses
from typing import List, Sequence


@dataclasses.dataclass
class EvaluationSuite:
  """seeds: the seeds to evaluate the agent on; max_episode_length: the most steps flown on one seed (> 0)."""
  seeds: Sequence[int]
  max_episode_length: int


_eval_suites = dict()
_eval_suites['big_eval'] = EvaluationSuite(list(range(10_000)), 960)
_eval_suites['medium_eval'] = EvaluationSuite(list(range(1_000)), 960)
_eval_suites['small_eval'] = EvaluationSuite(list(range(100)), 960)
_eval_suites['tiny_eval'] = EvaluationSuite(list(range(10)), 960)
_eval_suites['micro_eval'] = EvaluationSuite([0], 960)

# The strata suites are lists of seeds chosen by difficulty (the reference's eval/strata_seeds.py); the lists are not part of this
# package, so the names are known and refused.
STRATA_SUITES = tuple(f'{s}_strata' for s in ('hardest', 'hard', 'mid', 'easy', 'easiest')) + ('all_strata',)


def available_suites() -> List[str]:
  return list(_eval_suites.keys())


def get_eval_suite(name: str) -> EvaluationSuite:
  """Gets a named evaluation suite (a copy: the caller may change it)."""
  if name in STRATA_SUITES:
    raise NotImplementedError(f'eval suite {name}: the strata seed lists (the reference\'s eval/strata_seeds.py) are not part of this '
                              f'package; the range-based suites are {available_suites()}')
  if name not in _eval_suites:
    raise ValueError(f'Unknown eval suite {name}')
  suite = _eval_suites[name]
  return EvaluationSuite(list(suite.seeds), suite.max_episode_length)
