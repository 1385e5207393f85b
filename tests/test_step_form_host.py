"""ble_set_step_form's values on the host (no GPU: the switch is a process-global integer of the library): the helper form's value is
accepted and round-trips through _lib.step_form, 2 is still refused, and so is every value the library refused before."""
import pytest

from balloon_learning_environment_amd import _lib


def _lib_or_skip():
  try:
    return _lib.lib()
  except _lib.BleLibraryError as e:      # (the library is built by build(); without hipcc there is nothing to load)
    pytest.fail(f'libble_hip.so is not loadable: {e}')


def test_helper_form_value_round_trips():
  l = _lib_or_skip()
  assert _lib.STEP_FORM_HELPER == 12
  before = l.ble_set_step_form(0)
  try:
    with _lib.step_form(_lib.STEP_FORM_HELPER):
      assert l.ble_set_step_form(_lib.STEP_FORM_HELPER) == _lib.STEP_FORM_HELPER      # (returns the previous setting: the one just forced)
      with _lib.step_form(1):
        assert l.ble_set_step_form(1) == 1
      assert l.ble_set_step_form(_lib.STEP_FORM_HELPER) == _lib.STEP_FORM_HELPER      # restored by the inner block
    assert l.ble_set_step_form(0) == 0                                                  # restored by the outer block
  finally:
    l.ble_set_step_form(before)


@pytest.mark.parametrize('value', [2, 3, 5, 8, 11, 13, 16, 24, 64, -1, -12, 1 << 20])
def test_other_values_stay_refused(value):
  l = _lib_or_skip()
  before = l.ble_set_step_form(0)
  try:
    assert l.ble_set_step_form(value) < 0
    assert l.ble_set_step_form(0) == 0          # a refused value leaves the setting alone
    with pytest.raises(ValueError):
      with _lib.step_form(value):
        pass
  finally:
    l.ble_set_step_form(before)
