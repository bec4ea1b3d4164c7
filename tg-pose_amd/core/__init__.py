"""Drop-in pieces of the reference's ``core`` package that run on the device."""
