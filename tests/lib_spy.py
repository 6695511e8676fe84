"""The call counter of the GPU tests that assert which C-ABI entry points a route of the propagators took."""


class LibSpy(object):
    """Stands in for ``propagators.lib`` until ``monkeypatch.undo()``: ``seen[name]`` counts the calls the propagators module makes
    to entry point ``name`` -- of every entry point, or only of those in ``names``; the calls themselves go through unchanged."""

    def __init__(self, monkeypatch, names=None):
        from semiclassical_amd import propagators as PR
        self.real, self.seen, self.names = PR.lib, {}, names
        monkeypatch.setattr(PR, "lib", self)

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if self.names is not None and name not in self.names:
            return fn

        def counted(*a):
            self.seen[name] = self.seen.get(name, 0) + 1
            return fn(*a)
        return counted
