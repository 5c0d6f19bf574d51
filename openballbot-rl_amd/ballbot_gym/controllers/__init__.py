"""Controllers (the reference's ballbot_gym/controllers): the PID balance controller, its batched
form on the GPU and the install check `python -m ballbot_gym.controllers`."""
from .pid import PID, BatchedPID, balance


def main(argv=None) -> int:
    """The install check (scripts/test_pid.py of the reference); see __main__.py."""
    from .__main__ import main as _main

    return _main(argv)


__all__ = ["PID", "BatchedPID", "balance", "main"]
