"""The TP_* runtime switches in tests.  A switch read once per process is tested in child processes:
run_child / run_children start tests/<script> with the caller's environment minus every switch of engine.switch_table(),
plus the setting under test; the script's own side is child_main.  A switch read at every set-up is set in-process by
setup_env.  Every name is checked against the table, so a misspelt switch fails instead of testing the default twice."""
import contextlib
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):             # a child script run as `python tests/<script>` imports the package and its test modules
    if _p not in sys.path:
        sys.path.insert(0, _p)

MAX_CHILDREN = 4                    # side by side; the shared GPU machines allow 16 processes with the GPU open
_CACHE = {}


def table():
    """name -> entry of engine.switch_table()."""
    from thermalporous_amd import engine
    return {e["name"]: e for e in engine.switch_table()}


def child_env(env):
    """The caller's environment without any library switch, then `env`; every key of `env` must be a switch."""
    names = table()
    unknown = sorted(set(env) - set(names))
    assert not unknown, "not in engine.switch_table(): %s" % unknown
    full = {k: v for k, v in os.environ.items() if k not in names}
    full.update(env)
    return full


def _start(script, env, out, args):
    argv = [sys.executable, os.path.join(HERE, script)] + ([str(out)] if out is not None else []) + [str(a) for a in args]
    return subprocess.Popen(argv, env=child_env(env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _finish(proc, what, out, timeout):
    try:
        so, se = proc.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        proc.kill()
        proc.communicate()
        raise
    print(so[-3000:], end="")           # the child's figures, in the parent's captured output
    assert proc.returncode == 0 and so.strip().endswith("ok"), (what, so[-2000:], se[-2000:])
    if out is None:
        return so
    with np.load(str(out)) as z:
        return {k: z[k] for k in z.files}


def run_child(script, env, out=None, args=(), timeout=300, cache=False):
    """tests/<script> [out] [args...] as a fresh process under child_env(env): exit status 0 and a final "ok" asserted, the
    end of its output printed.  Returns the .npz the child wrote to `out` as a dict, or without `out` the child's stdout.
    cache: one run per (script, env, args)."""
    key = (script, tuple(sorted(env.items())), tuple(args))
    if cache and key in _CACHE:
        return _CACHE[key]
    res = _finish(_start(script, env, out, args), (script, env), out, timeout)
    if cache:
        _CACHE[key] = res
    return res


def run_children(script, settings, outdir, args=(), timeout=600):
    """run_child for every (name, env) of `settings`, side by side: all started, then each waited for.  The child of `name`
    writes outdir/<name>.npz; returns name -> that file as a dict."""
    assert len(settings) <= MAX_CHILDREN, "%d children side by side (at most %d)" % (len(settings), MAX_CHILDREN)
    for env in settings.values():           # every name checked before anything starts
        child_env(env)
    outs = {name: os.path.join(str(outdir), name + ".npz") for name in settings}
    procs = {}
    try:
        for name, env in settings.items():
            procs[name] = _start(script, env, outs[name], args)
        return {name: _finish(p, (script, name), outs[name], timeout) for name, p in procs.items()}
    finally:                                # one child failed or ran out of time: the others do not go on using the GPU
        for p in procs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()


@contextlib.contextmanager
def setup_env(**env):
    """Switches the library reads at every set-up, set while a hierarchy is built and put back afterwards.  A switch read
    once per process is refused: set in-process it would test nothing."""
    names = table()
    for k in env:
        assert k in names, "not in engine.switch_table(): %s" % k
        assert names[k]["when"] == "setup", "%s is read once per process: use run_child" % k
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def child_main(fn):
    """A child script's `if __name__ == "__main__"`: fn() runs the cases; the dict it returns (if any) goes to the .npz named
    by argv[1]; then the final "ok" the parent waits for."""
    out = fn()
    if out is not None:
        np.savez(sys.argv[1], **out)
    print("ok")
