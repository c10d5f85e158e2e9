"oracle/ref build (no source version)\n"
