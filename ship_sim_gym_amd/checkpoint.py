"""Checkpoint files: one ``torch.save`` of plain data, written atomically and read with ``weights_only=True``.

A file is ``{"format": "ssg-checkpoint", "version": 1, **sections}``.  The sections are the ``state_dict()`` of the objects a trainer
holds — every one of them returns only CPU tensors, ints, floats, bools, strings, lists and dicts, so no class is pickled and a file
can be read without trusting it:

    policy | population   NativePolicy.state_dict() or NativePopulation.state_dict()        (exactly one of the two)
    trainer               NativePPO.state_dict() or PopulationPPO.state_dict()
    obs_filter            ObsFilter.state_dict()
    ret_filter            ReturnFilter.state_dict()
    episode_log           EpisodeLog.state_dict()
    env                   ShipVecEnv.snapshot()
    scheduler             PBTScheduler.state_dict()
    loop                  the trainer script's own state (the last finished update, its generator, its history, the best score)
    config                the trainer script's keyword arguments, which a resumed run must repeat

``save`` writes to ``path + ".tmp"`` and then ``os.replace``s it over ``path``: a job that is killed during a save leaves the previous
file whole (a rename inside one directory is atomic).  ``load`` refuses a file of another format, an unknown version and a missing
section by name.
"""
import os

from ._native import _torch

FORMAT = "ssg-checkpoint"
VERSION = 1
SECTIONS = ("policy", "population", "trainer", "obs_filter", "ret_filter", "episode_log", "env", "scheduler", "loop", "config")


def check_plain(obj, where="checkpoint"):
    """Raise TypeError, naming the place, unless obj holds only tensors, ints, floats, bools, strings, lists and dicts with string
    keys — what every section is made of, and all that ``load`` is willing to read."""
    torch = _torch()
    if isinstance(obj, (bool, int, float, str)) or torch.is_tensor(obj):
        return obj
    if isinstance(obj, list):
        for i, v in enumerate(obj):
            check_plain(v, "%s[%d]" % (where, i))
        return obj
    if isinstance(obj, dict):
        for k, v in obj.items():
            if not isinstance(k, str):
                raise TypeError("%s: the key %r is a %s; keys must be strings" % (where, k, type(k).__name__))
            check_plain(v, "%s[%r]" % (where, k))
        return obj
    raise TypeError("%s is a %s; a checkpoint holds only tensors, ints, floats, bools, strings, lists and dicts" % (where, type(obj).__name__))


def is_checkpoint(obj):
    """True for what ``load`` returns and for a file's content that claims this format (whatever its version)."""
    return isinstance(obj, dict) and obj.get("format") == FORMAT


def save(path, sections):
    """Write the sections to `path` atomically.  sections: {name: state}, names out of SECTIONS, with ``policy`` or ``population``
    among them.  Nothing is left at ``path + ".tmp"``, whether the write succeeds or fails; a failure leaves `path` as it was."""
    torch = _torch()
    path = os.fspath(path)
    sections = dict(sections)
    for name in sections:
        if name not in SECTIONS:
            raise ValueError("checkpoint.save: unknown section %r (the sections are %s)" % (name, ", ".join(SECTIONS)))
    if ("policy" in sections) == ("population" in sections):
        raise ValueError("checkpoint.save: a file holds a 'policy' section or a 'population' section, one of the two")
    payload = {"format": FORMAT, "version": VERSION}
    payload.update(sections)
    check_plain(payload)
    tmp = path + ".tmp"
    try:
        torch.save(payload, tmp)
        os.replace(tmp, path)
    except BaseException:
        try:
            os.remove(tmp)
        except OSError:
            pass
        raise
    return path


def validate(obj, require=(), path="checkpoint"):
    """The checks of ``load`` on a file's content that was read already; returns it."""
    if not isinstance(obj, dict) or "format" not in obj:
        raise ValueError("%s: not a checkpoint (no 'format' entry; expected %r)" % (path, FORMAT))
    if obj["format"] != FORMAT:
        raise ValueError("%s: format %r, expected %r" % (path, obj["format"], FORMAT))
    if obj.get("version") != VERSION:
        raise ValueError("%s: version %r is not known to this library (it reads version %d)" % (path, obj.get("version"), VERSION))
    if ("policy" in obj) == ("population" in obj):
        raise ValueError("%s: a checkpoint holds a 'policy' section or a 'population' section, one of the two" % path)
    for name in require:
        if name not in obj:
            raise ValueError("%s: the section %r is missing (the file holds %s)"
                             % (path, name, ", ".join(k for k in SECTIONS if k in obj) or "no section"))
    return obj


def read(path):
    """What the file at `path` holds, on the CPU, read with ``weights_only=True`` (no code of the file's runs); not validated."""
    return _torch().load(os.fspath(path), map_location="cpu", weights_only=True)


def load(path, require=()):
    """Read a checkpoint: the dict ``save`` wrote, tensors on the CPU.  require: sections that must be there.  ValueError for another
    format, an unknown version, a file with neither or both of ``policy`` / ``population``, or a missing required section."""
    return validate(read(path), require, os.fspath(path))


def check_state(who, sd, fields=(), tensors=()):
    """What every ``load_state_dict`` does before it copies anything: ValueError unless `sd` is a dict in which every (name, value) of
    `fields` is present and equal to this object's value, and every (name, tensor) of `tensors` is present as a tensor of this
    object's tensor's shape and dtype.  The message names each offending field with both values."""
    torch = _torch()
    if not isinstance(sd, dict):
        raise ValueError("%s: a state dict is a dict (got a %s)" % (who, type(sd).__name__))
    bad = []
    for name, mine in fields:
        if name not in sd:
            bad.append("%s is missing (this object's is %r)" % (name, mine))
        elif torch.is_tensor(sd[name]):
            bad.append("%s is a tensor (this object's is %r)" % (name, mine))
        elif sd[name] != mine:
            bad.append("%s is %r in the state and %r in this object" % (name, sd[name], mine))
    for name, mine in tensors:
        t = sd.get(name)
        if not torch.is_tensor(t):
            bad.append("%s is %s (this object's is a %s tensor %s)" % (name, "missing" if t is None else "a " + type(t).__name__,
                                                                      mine.dtype, tuple(mine.shape)))
        elif tuple(t.shape) != tuple(mine.shape) or t.dtype != mine.dtype:
            bad.append("%s is a %s tensor %s in the state and a %s tensor %s in this object"
                       % (name, t.dtype, tuple(t.shape), mine.dtype, tuple(mine.shape)))
    if bad:
        raise ValueError("%s: %s" % (who, "; ".join(bad)))
    return sd


def check_values(who, sd, kinds):
    """ValueError unless every (name, type or tuple of types) of `kinds` is present in `sd` with a value of that type (a bool is not
    taken for a number): the fields a ``load_state_dict`` takes over instead of comparing."""
    bad = []
    for name, kind in kinds:
        if name not in sd:
            bad.append("%s is missing" % name)
        elif not isinstance(sd[name], kind) or (isinstance(sd[name], bool) and kind is not bool):
            bad.append("%s is a %s (%r)" % (name, type(sd[name]).__name__, sd[name]))
    if bad:
        raise ValueError("%s: %s" % (who, "; ".join(bad)))
    return sd


def config_differences(saved, current, exempt=()):
    """The keys (sorted) in which two ``config`` sections differ, leaving out `exempt`; a key only one of them has differs."""
    keys = (set(saved) | set(current)) - set(exempt)
    missing = object()
    return sorted(k for k in keys if saved.get(k, missing) != current.get(k, missing))


def plain_config(kwargs):
    """A trainer's keyword arguments as a ``config`` section: numbers, bools and strings as they are, None as the string "None",
    lists and tuples as lists, dicts by value, anything else by its ``repr``."""
    def conv(v):
        if isinstance(v, (bool, int, float, str)):
            return v
        if v is None:
            return "None"
        if isinstance(v, (list, tuple)):
            return [conv(x) for x in v]
        if isinstance(v, dict):
            return {str(k): conv(x) for k, x in sorted(v.items(), key=lambda kv: str(kv[0]))}
        if isinstance(v, type):
            return "%s.%s" % (v.__module__, v.__qualname__)
        return repr(v)
    return {str(k): conv(v) for k, v in kwargs.items()}
