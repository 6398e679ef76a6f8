"""``CompositeOptimizer``: different optimizers on different subsets of a model's parameters
(``experimental/optimizers/composite_optimizer.py``) -- e.g. ``ClippyAdagrad`` or ``Adagrad`` on the embedding tables,
which take the lookups' ``(ids, rows)`` slices, and another optimizer on the dense weights, as the ranking model's
docstring recommends (``experimental/models/ranking.py:243-246``).

A torch optimizer owns its parameters (``param_groups``), so each pair is ``(optimizer instance, callable returning
the parameters it handles)`` and the callable's set must be the optimizer's own; ``step()`` / ``zero_grad()`` fan out,
``apply_gradients`` is the reference-shaped entry.
"""

from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import torch


class CompositeOptimizer:

  def __init__(self, optimizers_and_vars: Sequence[Tuple[torch.optim.Optimizer, Callable[[], Iterable[torch.Tensor]]]],
               name: str = "CompositeOptimizer") -> None:
    if not optimizers_and_vars:
      raise ValueError("`optimizers_and_vars` can't be empty")
    self._optimizers_and_vars = list(optimizers_and_vars)
    self.name = name
    self._checked = False

  @property
  def optimizers(self) -> List[torch.optim.Optimizer]:
    """The member optimizers, in the original order."""
    return [optimizer for optimizer, _ in self._optimizers_and_vars]

  # -- consistency -------------------------------------------------------------------------------------------------
  def _owner_by_param(self) -> Dict[int, torch.optim.Optimizer]:
    """id(parameter) -> member; raises when two members are given the same parameter or a callable's set is not its
    optimizer's own."""
    owner: Dict[int, torch.optim.Optimizer] = {}
    for optimizer, var_callable in self._optimizers_and_vars:
      listed = list(var_callable())
      for v in listed:
        if id(v) in owner:
          raise ValueError(
              f"The set of variables handled by each optimizer should be disjoint, but variable of shape "
              f"{tuple(v.shape)} is handled both by {type(owner[id(v)]).__name__} and {type(optimizer).__name__}.")
        owner[id(v)] = optimizer
      own = {id(p) for group in optimizer.param_groups for p in group["params"]}
      if own != {id(v) for v in listed}:
        raise ValueError(
            f"{type(optimizer).__name__} was built on {len(own)} parameters but its callable returns "
            f"{len(listed)}: the callable must return exactly the parameters the optimizer was built on.")
    return owner

  def validate(self, trainable_params: Optional[Iterable[torch.Tensor]] = None) -> None:
    """The checks of the first step; with ``trainable_params`` (``Model`` passes its own before the first step after
    ``compile``) additionally: every one of them is handled by some member."""
    owner = self._owner_by_param()
    for v in (trainable_params or ()):
      if v.requires_grad and id(v) not in owner:
        raise ValueError(f"Variable of shape {tuple(v.shape)} is not handled by any optimizer. "
                         f"This would cause it to be not trained.")
    self._checked = True

  def _check_gradients_have_owners(self, params: Iterable[torch.Tensor], owner) -> None:
    for v in params:
      if id(v) not in owner:
        raise ValueError(f"Variable of shape {tuple(v.shape)} is not handled by any optimizer. "
                         f"This would cause it to be not trained.")

  # -- the optimizer surface `Model` uses --------------------------------------------------------------------------
  def step(self, closure=None):
    loss = None
    if closure is not None:
      with torch.enable_grad():
        loss = closure()
    if not self._checked:
      self.validate()
    for optimizer in self.optimizers:
      optimizer.step()
    return loss

  def zero_grad(self, set_to_none: bool = True) -> None:
    for optimizer in self.optimizers:
      optimizer.zero_grad(set_to_none=set_to_none)

  def apply_gradients(self, grads_and_vars) -> None:
    """``grads_and_vars``: pairs ``(gradient, parameter)``; a gradient is a tensor or the ``(ids, rows)`` slices of an
    embedding lookup (``tf.IndexedSlices``), which need a member that takes slices on that parameter."""
    grads_and_vars = list(grads_and_vars)
    owner = self._owner_by_param()
    self._check_gradients_have_owners([v for _, v in grads_and_vars], owner)
    self._checked = True
    for g, v in grads_and_vars:
      if isinstance(g, (tuple, list)):
        if not getattr(v, "_tfrs_sparse_grad", False):
          raise ValueError(f"(ids, rows) slices for a variable of shape {tuple(v.shape)} whose optimizer "
                           f"({type(owner[id(v)]).__name__}) does not take slices")
        v._tfrs_slices.append((g[0], g[1]))
      else:
        v.grad = g
    for optimizer in self.optimizers:
      optimizer.step()

  @property
  def param_groups(self) -> List[dict]:
    """The members' own group dicts (a change of a hyper-parameter through them reaches the member)."""
    return [group for optimizer in self.optimizers for group in optimizer.param_groups]

  @property
  def state(self) -> Dict:
    out = {}
    for optimizer in self.optimizers:
      out.update(optimizer.state)
    return out

  def state_dict(self) -> Dict:
    return {"optimizers": [optimizer.state_dict() for optimizer in self.optimizers]}

  def load_state_dict(self, state_dict: Dict) -> None:
    members = state_dict["optimizers"]
    if len(members) != len(self._optimizers_and_vars):
      raise ValueError(f"state of {len(members)} optimizers for a composite of {len(self._optimizers_and_vars)}")
    for optimizer, member in zip(self.optimizers, members):
      optimizer.load_state_dict(member)

  def reset_state_(self) -> None:
    """Every member's state back to its initial value in place; members without ``reset_state_`` (plain
    ``torch.optim``) are left as they are."""
    for optimizer in self.optimizers:
      fn = getattr(optimizer, "reset_state_", None)
      if callable(fn):
        fn()

  def capture_rollback(self):
    """What ``Model`` calls before the warm-up iterations of a graph capture: a callable that puts every member's state
    back IN PLACE afterwards (a captured step writes into this very storage), or ``None`` when some member cannot be
    put back.  Member by member: state that exists now is snapshotted and copied back; a member without state yet is
    re-initialised through its ``reset_state_``; a member with neither (a plain ``torch.optim`` optimizer whose state
    is created lazily by the warm-up) makes the whole composite answer ``None`` -- the warm-up iterations then stay
    applied as ordinary training steps for ALL members and the parameters, never for some of them."""
    saved, resets = [], []
    for optimizer in self.optimizers:
      tensors = [t for st in optimizer.state.values() for t in st.values() if isinstance(t, torch.Tensor)]
      # (both for a member with a learning-rate schedule: its counter exists from the constructor on, its accumulators
      # are created by the warm-up -- those are re-initialised first, what existed is then copied back over it)
      if callable(getattr(optimizer, "reset_state_", None)):
        resets.append(optimizer.reset_state_)
      elif not tensors:
        return None
      saved.extend((t, t.detach().clone()) for t in tensors)

    def roll_back():
      for fn in resets:
        fn()
      with torch.no_grad():
        for t, v in saved:
          t.copy_(v)

    return roll_back

  def bump_table_versions(self) -> None:
    for optimizer in self.optimizers:
      fn = getattr(optimizer, "bump_table_versions", None)
      if callable(fn):
        fn()

  def close(self) -> None:
    for optimizer in self.optimizers:
      fn = getattr(optimizer, "close", None)
      if callable(fn):
        fn()

  def get_config(self):
    raise NotImplementedError("CompositeOptimizer cannot be serialized because it uses callable to get variables.")
