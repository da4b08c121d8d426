"""Kaldi conf files and the option sets read from them: `--name=value` lines, options known by their Kaldi names, and what a program does not
implement refused by name.  MfccOptions / FbankOptions / VadOptions (features.py) and AugmentOptions (augment.py) are such sets."""
_TRUE, _FALSE = ("true", "t", "1"), ("false", "f", "0")


def _bool(name, text):
    if text.lower() in _TRUE:
        return 1
    if text.lower() in _FALSE:
        return 0
    raise ValueError("--%s=%s: true or false is expected" % (name, text))


def _conf_lines(path):
    """(name, value) of every `--name=value` line of a Kaldi conf file; `#` starts a comment."""
    out = []
    with open(path, "r") as f:
        for number, line in enumerate(f, 1):
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            if not line.startswith("--") or "=" not in line:
                raise ValueError("%s:%d: `--name=value` is expected, got `%s`" % (path, number, line))
            name, value = line[2:].split("=", 1)
            out.append((name.strip(), value.strip()))
    return out


class _Options(object):
    """Options by Kaldi name.  SUPPORTED: name -> (attribute, parser).  FIXED: options of the Kaldi program that this one does not
    implement, name -> (the one value that changes nothing, parser): that value is accepted, any other is refused by name."""
    SUPPORTED, FIXED, PROGRAM = {}, {}, ""

    def __init__(self, **kw):
        for attr, _ in self.SUPPORTED.values():
            setattr(self, attr, self.DEFAULTS[attr])
        for k, v in kw.items():
            if k not in self.DEFAULTS:
                raise TypeError("%s: no option `%s`" % (type(self).__name__, k))
            setattr(self, k, v)

    def set(self, name, text):
        if name in self.SUPPORTED:
            attr, parse = self.SUPPORTED[name]
            setattr(self, attr, parse(name, text))
        elif name in self.FIXED:
            only, parse = self.FIXED[name]
            if parse(name, text) != only:
                raise ValueError("--%s=%s is not supported (only --%s=%s: %s)" % (name, text, name, str(only).lower(), self.WHY.get(name, "not implemented")))
        else:
            raise ValueError("--%s is not an option of %s that this program knows" % (name, self.PROGRAM))

    @classmethod
    def from_conf(cls, path):
        self = cls()
        for name, value in _conf_lines(path):
            self.set(name, value)
        return self


def _f(name, text):
    try:
        return float(text)
    except ValueError:
        raise ValueError("--%s=%s: a number is expected" % (name, text))


def _i(name, text):
    try:
        return int(text)
    except ValueError:
        raise ValueError("--%s=%s: a whole number is expected" % (name, text))


def _s(name, text):
    return text
