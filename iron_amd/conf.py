"""A reader for the settings files of stage 1 (confs/*.conf, which render_volume.py reads through pyhocon) without pyhocon.

The grammar is what those files use and nothing more:

    name { ... }                 nested blocks
    key = value                  entries, with an optional comma behind them (`D = 8,`)
    # ...                        comments to the end of the line, also behind a value
    [a, b]                       lists, which may span lines
    12, 5e-4, True / False / true / false, "quoted strings", unquoted strings (./exp_stage1/CASE_NAME/, idr, blender_0.1)

Everything else -- substitutions (${...}), `include`, `+=`, dotted keys, a brace that never closes -- raises ConfError with the
number of the line.  `parse_string` takes the text after the caller has replaced CASE_NAME, as render_volume.py:30-34 does.

The result is a Conf: a dict whose keys may be dotted paths (conf["train.end_iter"], "model.nerf" in conf), with pyhocon's
get_int / get_float / get_bool / get_string (each with default=), and whose blocks unpack as keyword arguments
(NeRF(**conf["model.nerf"])).
"""
from __future__ import annotations

import re

_MISSING = object()
_KEY = re.compile(r"[A-Za-z_][A-Za-z0-9_\-]*")
_INT = re.compile(r"[+-]?[0-9]+\Z")
_FLOAT = re.compile(r"[+-]?([0-9]+\.[0-9]*|\.[0-9]+|[0-9]+)([eE][+-]?[0-9]+)?\Z")


class ConfError(ValueError):
    pass


class Conf(dict):
    """A block of a settings file.  Keys may be dotted paths through nested blocks."""

    def _walk(self, key):
        node = self
        for part in str(key).split("."):
            if not isinstance(node, dict) or not dict.__contains__(node, part):
                return _MISSING
            node = dict.__getitem__(node, part)
        return node

    def __getitem__(self, key):
        v = self._walk(key)
        if v is _MISSING:
            raise KeyError(key)
        return v

    def __contains__(self, key):
        return self._walk(key) is not _MISSING

    def __setitem__(self, key, value):
        *path, last = str(key).split(".")
        node = self
        for part in path:
            if not dict.__contains__(node, part):
                dict.__setitem__(node, part, Conf())
            node = dict.__getitem__(node, part)
            if not isinstance(node, dict):
                raise ConfError("%s: %r is not a block" % (key, part))
        dict.__setitem__(node, last, value)

    def get(self, key, default=None):
        v = self._walk(key)
        return default if v is _MISSING else v

    def _typed(self, key, default, kind, convert):
        v = self._walk(key)
        if v is _MISSING:
            if default is _MISSING:
                raise ConfError("no entry %r" % (key,))
            return default
        try:
            return convert(v)
        except (TypeError, ValueError):
            raise ConfError("%s = %r is not %s" % (key, v, kind)) from None

    def get_int(self, key, default=_MISSING):
        def convert(v):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError
            return v
        return self._typed(key, default, "an integer", convert)

    def get_float(self, key, default=_MISSING):
        def convert(v):
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError
            return float(v)
        return self._typed(key, default, "a number", convert)

    def get_bool(self, key, default=_MISSING):
        def convert(v):
            if not isinstance(v, bool):
                raise ValueError
            return v
        return self._typed(key, default, "True or False", convert)

    def get_string(self, key, default=_MISSING):
        def convert(v):
            if isinstance(v, (dict, list)):
                raise ValueError
            return str(v)
        return self._typed(key, default, "a string", convert)


def _scalar(text, line):
    if "${" in text:
        raise ConfError("line %d: substitutions (${...}) are not supported" % line)
    if text in ("True", "true"):
        return True
    if text in ("False", "false"):
        return False
    if _INT.match(text):
        return int(text)
    if _FLOAT.match(text):
        return float(text)
    return text


class _Parser:
    def __init__(self, text):
        self.s, self.i, self.line = text, 0, 1

    def fail(self, what, line=None):
        raise ConfError("line %d: %s" % (self.line if line is None else line, what))

    def skip(self, commas=False):
        """White space, comments and (between entries) commas."""
        s = self.s
        while self.i < len(s):
            c = s[self.i]
            if c == "\n":
                self.line += 1
                self.i += 1
            elif c in " \t\r" or (commas and c == ","):
                self.i += 1
            elif c == "#":
                while self.i < len(s) and s[self.i] != "\n":
                    self.i += 1
            else:
                break

    def quoted(self):
        start, s = self.line, self.s
        self.i += 1
        out = []
        while True:
            if self.i >= len(s) or s[self.i] == "\n":
                self.fail("the quoted string does not end on its line", start)
            c = s[self.i]
            self.i += 1
            if c == '"':
                return "".join(out)
            if c == "\\":
                if self.i >= len(s):
                    self.fail("the quoted string does not end on its line", start)
                c = {"n": "\n", "t": "\t"}.get(s[self.i], s[self.i])
                self.i += 1
            out.append(c)

    def value(self, in_list):
        s = self.s
        if self.i >= len(s):
            self.fail("a value is missing")
        c = s[self.i]
        if c == "[":
            return self.list()
        if c == "{":
            self.fail("a block is written `name { ... }`, not as a value")
        if c == '"':
            return self.quoted()
        j = self.i
        stop = "\n#,]" if in_list else "\n#,}"
        while j < len(s) and s[j] not in stop:
            j += 1
        text = s[self.i:j].strip()
        self.i = j
        if not text:
            self.fail("a value is missing")
        return _scalar(text, self.line)

    def list(self):
        start = self.line
        self.i += 1
        out = []
        while True:
            self.skip(commas=True)
            if self.i >= len(self.s):
                self.fail("the list opened here is never closed", start)
            if self.s[self.i] == "]":
                self.i += 1
                return out
            out.append(self.value(in_list=True))

    def block(self, opened_at):
        out = Conf()
        s = self.s
        while True:
            self.skip(commas=True)
            if self.i >= len(s):
                if opened_at is not None:
                    self.fail("the brace opened here is never closed", opened_at)
                return out
            if s[self.i] == "}":
                if opened_at is None:
                    self.fail("a closing brace without a block")
                self.i += 1
                return out
            m = _KEY.match(s, self.i)
            if not m:
                self.fail("expected a name, found %r" % s[self.i])
            key, key_line = m.group(0), self.line
            self.i = m.end()
            if key == "include":
                self.fail("`include` is not supported")
            while self.i < len(s) and s[self.i] in " \t":
                self.i += 1
            c = s[self.i] if self.i < len(s) else ""
            if c == "{":
                self.i += 1
                value = self.block(key_line)
            elif c == "=" or c == ":":
                self.i += 1
                while self.i < len(s) and s[self.i] in " \t":
                    self.i += 1
                value = self.value(in_list=False)
            elif s.startswith("+=", self.i):
                self.fail("`+=` is not supported")
            elif c == ".":
                self.fail("dotted names are not supported; nest the blocks")
            else:
                self.fail("expected `=` or `{` after %r" % key)
            if dict.__contains__(out, key):
                self.fail("%r is set twice in one block" % key, key_line)
            dict.__setitem__(out, key, value)


def parse_string(text) -> Conf:
    return _Parser(text).block(None)


def parse_file(path, case=None) -> Conf:
    """The file's text with CASE_NAME replaced by `case` (render_volume.py:30-34), parsed."""
    with open(path) as f:
        text = f.read()
    return parse_string(text if case is None else text.replace("CASE_NAME", case))
