"""Stand-in child of tests/test_switches_host.py: reports the TP_* variables it was started with.  No GPU."""
import os

from switches import child_main

if __name__ == "__main__":
    child_main(lambda: dict(names=[k for k in sorted(os.environ) if k.startswith("TP_")],
                            values=[os.environ[k] for k in sorted(os.environ) if k.startswith("TP_")]))
