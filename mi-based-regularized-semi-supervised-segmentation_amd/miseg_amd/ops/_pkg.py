"""What the family modules read from the ``ops`` namespace at the moment they run, so that one assignment from outside -- a launch
spy's ``monkeypatch.setattr(ops, "call", spy)``, a test's ``ops._MI_PLANES = True`` -- reaches every family."""
import sys


def call(name, *args, **kwargs):
    return sys.modules[__package__].call(name, *args, **kwargs)


def mi_planes() -> bool:
    return sys.modules[__package__]._MI_PLANES
