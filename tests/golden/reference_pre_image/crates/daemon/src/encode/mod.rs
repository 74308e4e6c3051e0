

pub mod av1an;

pub use av1an::{build_av1an_command, run_av1an, Av1anEncodeParams, EncodeError};
